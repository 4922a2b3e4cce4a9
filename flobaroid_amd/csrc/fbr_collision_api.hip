// fbr_collision_api.hip -- the collision entry points of the C-ABI (include/fbr.h): the capsule, box and convex-hull sets, the triangle
// meshes attached to hulls, their candidate distances and their distance gradients.  The kernels are those of fbr_capsule.h, fbr_box.h,
// fbr_hull.h, fbr_mesh.h, fbr_mesh_bvh.h and their *_grad.h siblings (section FBR_KERNELS_COLLISION); the tables every set shares are built by
// fbr_collision_tables.h.  DESIGN.md, "collision layout".
#define FBR_KERNELS_COLLISION
#include "fbr_internal.h"
#include "fbr_hull_large_grad.h"
#include "fbr_mesh_bvh_grad.h"
#include <functional>
#include <limits>

// ---- what the three sets share -------------------------------------------------------------------------------------------------------
static int collision_program(const fbr_model *m, FbrKinIdProgram &prog)
{
    try {
        fbr_kinid_build(m->hm, prog);
    } catch (const std::exception &e) {
        set_err(e.what());
        return FBR_E_INVALID;
    }
    return FBR_OK;
}

// a set's packed arrays into its buffer (+ 8: the slack the int2 loads of the last pair may touch)
static int upload_blob(DevBuf &buf, const FbrBlob &blob)
{
    if (int rc = buf.ensure(blob.bytes.size() + 8)) return rc;
    HIPCHK(hipMemcpy(buf.p, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice));
    return FBR_OK;
}

// the table of a set's gradient call (fbr_collision_grad_table), in an allocation of its own
static int upload_grad_table(DevBuf &buf, const FbrCollisionSort &srt, const int32_t *link, int npairs, const int32_t *pairs, DevPairGrad *out)
{
    const std::vector<int> gt = fbr_collision_grad_table(srt, link, npairs, pairs);
    if (int rc = buf.ensure(gt.size() * sizeof(int))) return rc;
    HIPCHK(hipMemcpy(buf.p, gt.data(), gt.size() * sizeof(int), hipMemcpyHostToDevice));
    out->W = srt.W;
    out->pair = (const int4 *)buf.p;
    out->anc = buf.as<int>() + (size_t)4 * std::max(npairs, 1);
    return FBR_OK;
}

// ---- capsule collision set (csrc/fbr_capsule.h) ------------------------------------------------------------------------------------------
extern "C" int fbr_model_set_capsules(fbr_model *m, int32_t ncaps, const int32_t *link, const double *seg, const double *radius, int32_t npairs,
                                      const int32_t *pairs)
{
    if (!m) {
        set_err("null model");
        return FBR_E_INVALID;
    }
    if (ncaps < 0 || npairs < 0 || ncaps > FBR_MAX_CAPSULES || npairs > FBR_MAX_CAPSULE_PAIRS) {
        set_err("capsule set: at most " + std::to_string(FBR_MAX_CAPSULES) + " capsules and " + std::to_string(FBR_MAX_CAPSULE_PAIRS) + " pairs");
        return FBR_E_INVALID;
    }
    if ((ncaps > 0 && (!link || !seg || !radius)) || (npairs > 0 && !pairs)) {
        set_err("capsule set: null array");
        return FBR_E_INVALID;
    }
    const FbrHostModel &hm = m->hm;
    for (int c = 0; c < ncaps; c++) {
        if (link[c] < 0 || link[c] >= hm.L) {
            set_err("capsule " + std::to_string(c) + ": link index out of range");
            return FBR_E_INVALID;
        }
        if (!(radius[c] >= 0.0) || !std::isfinite(radius[c])) {
            set_err("capsule " + std::to_string(c) + ": the radius must be finite and not negative");
            return FBR_E_INVALID;
        }
        for (int i = 0; i < 6; i++)
            if (!std::isfinite(seg[6 * c + i])) {
                set_err("capsule " + std::to_string(c) + ": non-finite endpoint");
                return FBR_E_INVALID;
            }
    }
    for (int k = 0; k < npairs; k++) {
        const int a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a < 0 || a >= ncaps || b < 0 || b >= ncaps || a == b) {
            set_err("capsule pair " + std::to_string(k) + ": capsule index out of range, or a capsule paired with itself");
            return FBR_E_INVALID;
        }
    }
    if (int rc = enter_blocking(m)) return rc;  // (no launch that reads the tables replaced below is in flight)
    HIPCHK(hipStreamSynchronize(m->stream));
    // (unlike the box and the hull setter this one leaves capg as it is when the set is cleared: fbr_capsule_distance_gradients looks at
    // caps first and never reads the stale table)
    m->caps = DevCapsules{0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (ncaps == 0) return FBR_OK;
    FbrKinIdProgram prog;
    if (int rc = collision_program(m, prog)) return rc;
    FbrCollisionSort srt;
    fbr_collision_sort(hm, prog, ncaps, link, srt);  // (no world capsules: a capsule's number is its code, srt.id the caller's index of a slot)
    // one allocation: seg (by slot) | radius | steps | capbeg | capid | pairs
    FbrBlob blob;
    const size_t oseg = blob.add<double>((size_t)ncaps * 6), orad = blob.add<double>(radius, radius + ncaps);
    const size_t osteps = blob.add<int>(prog.steps.begin(), prog.steps.end()), obeg = blob.add<int>(srt.beg.begin(), srt.beg.end());
    const size_t oid = blob.add<int>(srt.id.begin(), srt.id.end()), opairs = blob.add<int>(2 * (size_t)std::max(npairs, 1), sizeof(int2));
    for (int c = 0; c < ncaps; c++) std::copy(seg + 6 * c, seg + 6 * c + 6, blob.at<double>(oseg) + (size_t)srt.slot[c] * 6);
    std::copy(pairs, pairs + 2 * (size_t)npairs, blob.at<int>(opairs));
    if (int rc = upload_blob(m->cap_tab, blob)) return rc;
    const char *base = (const char *)m->cap_tab.p;
    const DevCapsules dc = {prog.nsteps, prog.nslots, ncaps, npairs, (const int *)(base + osteps), (const int *)(base + obeg), (const int *)(base + oid),
                            (const double *)(base + oseg), (const double *)(base + orad), (const int2 *)(base + opairs)};
    if (int rc = upload_grad_table(m->capg_tab, srt, link, npairs, pairs, &m->capg)) return rc;
    m->caps = dc;
    return FBR_OK;
}

// ---- box collision set (csrc/fbr_box.h) ----------------------------------------------------------------------------------------------
extern "C" int fbr_model_set_boxes(fbr_model *m, int32_t nboxes, const int32_t *link, const double *half, const double *center, const double *rot,
                                   int32_t center_in_link_axes, int32_t npairs, const int32_t *pairs)
{
    if (!m) {
        set_err("null model");
        return FBR_E_INVALID;
    }
    if (nboxes < 0 || npairs < 0 || nboxes > FBR_MAX_BOXES || npairs > FBR_MAX_BOX_PAIRS) {
        set_err("box set: at most " + std::to_string(FBR_MAX_BOXES) + " boxes and " + std::to_string(FBR_MAX_BOX_PAIRS) + " pairs");
        return FBR_E_INVALID;
    }
    if ((nboxes > 0 && (!link || !half || !center)) || (npairs > 0 && !pairs)) {
        set_err("box set: null array");
        return FBR_E_INVALID;
    }
    const FbrHostModel &hm = m->hm;
    for (int c = 0; c < nboxes; c++) {
        if (link[c] < -1 || link[c] >= hm.L) {
            set_err("box " + std::to_string(c) + ": link index out of range (-1: a world box)");
            return FBR_E_INVALID;
        }
        for (int i = 0; i < 3; i++) {
            if (!(half[3 * c + i] > 0.0) || !std::isfinite(half[3 * c + i])) {
                set_err("box " + std::to_string(c) + ": the half extents must be finite and positive");
                return FBR_E_INVALID;
            }
            if (!std::isfinite(center[3 * c + i])) {
                set_err("box " + std::to_string(c) + ": non-finite centre");
                return FBR_E_INVALID;
            }
        }
        if (link[c] < 0) {
            if (!rot) {
                set_err("box " + std::to_string(c) + ": a world box needs rot");
                return FBR_E_INVALID;
            }
            for (int i = 0; i < 9; i++)
                if (!std::isfinite(rot[9 * c + i])) {
                    set_err("box " + std::to_string(c) + ": non-finite rotation");
                    return FBR_E_INVALID;
                }
        }
    }
    for (int k = 0; k < npairs; k++) {
        const int a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a < 0 || a >= nboxes || b < 0 || b >= nboxes || a == b) {
            set_err("box pair " + std::to_string(k) + ": box index out of range, or a box paired with itself");
            return FBR_E_INVALID;
        }
        if (link[a] < 0 && link[b] < 0) {
            set_err("box pair " + std::to_string(k) + ": two world boxes");
            return FBR_E_INVALID;
        }
    }
    if (int rc = enter_blocking(m)) return rc;  // (no launch that reads the tables replaced below is in flight)
    HIPCHK(hipStreamSynchronize(m->stream));
    m->boxes = kNoBoxes;
    m->boxg = DevPairGrad{0, nullptr, nullptr};
    if (nboxes == 0) return FBR_OK;
    FbrKinIdProgram prog;
    if (int rc = collision_program(m, prog)) return rc;
    FbrCollisionSort srt;
    fbr_collision_sort(hm, prog, nboxes, link, srt);
    // one allocation: cen (by slot) | half (by robot-box number) | world | steps | boxbeg | boxid | pairs (the boxes' codes)
    const size_t nr = (size_t)std::max(srt.nrob, 1), nw = (size_t)std::max(srt.nworld, 1);
    FbrBlob blob;
    const size_t ocen = blob.add<double>(nr * 3), ohalf = blob.add<double>(nr * 3), oworld = blob.add<double>(nw * 15);
    const size_t osteps = blob.add<int>(prog.steps.begin(), prog.steps.end()), obeg = blob.add<int>(srt.beg.begin(), srt.beg.end());
    const size_t oid = blob.add<int>(srt.id.begin(), srt.id.end()), opairs = blob.add<int>(2 * (size_t)std::max(npairs, 1), sizeof(int2));
    for (int c = 0; c < nboxes; c++) {
        if (link[c] >= 0) {
            std::copy(center + 3 * c, center + 3 * c + 3, blob.at<double>(ocen) + (size_t)srt.slot[c] * 3);
            std::copy(half + 3 * c, half + 3 * c + 3, blob.at<double>(ohalf) + (size_t)srt.code[c] * 3);
        } else {
            double *w = blob.at<double>(oworld) + (size_t)(-1 - srt.code[c]) * 15;
            std::copy(rot + 9 * c, rot + 9 * c + 9, w);
            std::copy(center + 3 * c, center + 3 * c + 3, w + 9);
            std::copy(half + 3 * c, half + 3 * c + 3, w + 12);
        }
    }
    for (size_t k = 0; k < 2 * (size_t)npairs; k++) blob.at<int>(opairs)[k] = srt.code[pairs[k]];
    if (int rc = upload_blob(m->box_tab, blob)) return rc;
    const char *base = (const char *)m->box_tab.p;
    const DevBoxes db = {prog.nsteps, prog.nslots, srt.nrob, srt.nworld, npairs, center_in_link_axes ? 1 : 0, (const int *)(base + osteps),
                         (const int *)(base + obeg), (const int *)(base + oid), (const double *)(base + ocen), (const double *)(base + ohalf),
                         (const double *)(base + oworld), (const int2 *)(base + opairs)};
    if (int rc = upload_grad_table(m->boxg_tab, srt, link, npairs, pairs, &m->boxg)) return rc;
    m->boxes = db;
    return FBR_OK;
}

// ---- convex-hull collision set (csrc/fbr_hull.h) -----------------------------------------------------------------------------------------
// The class views and the stencil tables of a hull set (fbr_hull_pair_classes, fbr_stencil_table of fbr_collision_tables.h) from the host's
// copy of the set and the mesh table (null: no meshes), into an allocation of their own: both setters build `out` beside what is installed
// and move it in once nothing can fail any more.
static int build_hull_views(const fbr_model *m, const DevHulls &set, const FbrHullSet::Host &hh, bool large_set, const int *mtab, int meshes,
                            FbrHullViews &out)
{
    const int npairs = set.npairs;
    const FbrPairClasses pc = fbr_hull_pair_classes(set.nhulls, hh.vbeg.data(), mtab, npairs, hh.pairs.data());
    // the stencil tables and the columns they cover: the MESH view (fbr_mesh_distance_gradients: small meshes, fbr_large_mesh_distance_gradients:
    // a tree attachment), the BIG view (a set of fbr_model_set_large_hulls without meshes or with a tree attachment) and every pair
    // (fbr_large_hull_distance_gradients with option hull_large_all: a set of fbr_model_set_large_hulls without meshes)
    std::vector<int> every((size_t)npairs);
    std::iota(every.begin(), every.end(), 0);
    const bool lgrad = large_set && meshes == FBR_MESHES_NONE && npairs > 0;
    const bool bgrad = large_set && meshes != FBR_MESHES_SMALL && npairs > 0;
    const std::vector<int> *cols[3] = {meshes != FBR_MESHES_NONE ? &pc.col[FBR_PAIR_MESH] : nullptr,
                                       bgrad && !pc.col[FBR_PAIR_BIG].empty() ? &pc.col[FBR_PAIR_BIG] : nullptr, lgrad ? &every : nullptr};
    FbrStencilTable st[3];
    if (cols[0] || cols[1] || cols[2]) {
        FbrKinIdProgram prog;
        if (int rc = collision_program(m, prog)) return rc;
        std::vector<int> stepof, anc;
        fbr_capgrad_ancestors(m->hm, prog, stepof, anc);
        for (int i = 0; i < 3; i++)
            if (cols[i])
                st[i] = fbr_stencil_table(*cols[i], hh.link.data(), stepof.data(), anc.data(), fbr_capgrad_words(prog.nsteps), set.fr.cmode,
                                          prog.steps.data(), hh.pairs.data());
    }
    // one allocation: the pairs of the classes | their columns | the stencil tables
    FbrBlob blob;
    size_t op[FBR_PAIR_CLASSES], oc[FBR_PAIR_CLASSES], os[3];
    for (int c = 0; c < FBR_PAIR_CLASSES; c++) op[c] = blob.add<int>(pc.pairs[c].begin(), pc.pairs[c].end(), sizeof(int2));
    for (int c = 0; c < FBR_PAIR_CLASSES; c++) oc[c] = blob.add<int>(pc.col[c].begin(), pc.col[c].end());
    for (int i = 0; i < 3; i++) os[i] = blob.add<int>(st[i].tab.begin(), st[i].tab.end());
    if (int rc = upload_blob(out.tab, blob)) return rc;
    const char *base = (const char *)out.tab.p;
    for (int c = 0; c < FBR_PAIR_CLASSES; c++) {
        const int cnt = (int)pc.col[c].size();
        // (a class that covers every pair of a set without meshes is the whole set, in the caller's columns)
        const bool whole = mtab == nullptr && cnt == npairs;
        out.view[c].npairs = cnt;
        out.view[c].pairs = whole ? set.pairs : (const int2 *)(base + op[c]);
        out.view[c].col = whole ? nullptr : (const int *)(base + oc[c]);
    }
    FbrStencil *dst[3] = {&out.mesh, &out.big, &out.all};
    for (int i = 0; i < 3; i++) {
        const int *g = (const int *)(base + os[i]);
        if (!cols[i]) continue;  // (out is the caller's fresh one: an empty table)
        dst[i]->dev = DevMeshGrad{st[i].nitems, st[i].smax, g, g + st[i].npairs + 1, g + st[i].npairs + 1 + st[i].nitems};
        dst[i]->sbeg.assign(st[i].tab.begin(), st[i].tab.begin() + st[i].npairs + 1);
    }
    return FBR_OK;
}

// fbr_model_set_hulls (max_vertices FBR_MAX_HULL_VERTICES) and fbr_model_set_large_hulls (FBR_MAX_LARGE_HULL_VERTICES, large): one set, two caps
static int install_hulls(fbr_model *m, int max_vertices, bool large, int32_t nhulls, const int32_t *link, const double *offset, const double *rot,
                         int32_t offset_in_link_axes, const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes,
                         const int32_t *ebeg, const int32_t *edges, int32_t npairs, const int32_t *pairs)
{
    if (!m) {
        set_err("null model");
        return FBR_E_INVALID;
    }
    const FbrHostModel &hm = m->hm;
    std::vector<double> diam((size_t)std::max(std::min(nhulls, FBR_MAX_HULLS), 1), 0.0);
    const std::string bad = fbr_hull_validate(hm.L, FBR_MAX_HULLS, FBR_MAX_HULL_PAIRS, max_vertices, nhulls, link, offset, rot, vbeg, verts, fbeg, planes, ebeg,
                                              edges, npairs, pairs, diam.data());
    if (!bad.empty()) {
        set_err(bad);
        return FBR_E_INVALID;
    }
    if (int rc = enter_blocking(m)) return rc;  // (no launch that reads the tables replaced below is in flight)
    HIPCHK(hipStreamSynchronize(m->stream));
    m->hs.clear();  // (the meshes attached to the set before are gone with it: fbr_model_set_hull_meshes)
    if (nhulls == 0) return FBR_OK;
    FbrKinIdProgram prog;
    if (int rc = collision_program(m, prog)) return rc;
    FbrCollisionSort srt;  // (the robot hulls by slot, as the robot boxes are: the frames kernel walks them)
    fbr_collision_sort(hm, prog, nhulls, link, srt);
    // one allocation: cen (by slot) | diam | world | verts | planes | steps | beg | slot ids | tab | edges | pairs (the caller's numbers)
    const size_t nr = (size_t)std::max(srt.nrob, 1), nw = (size_t)std::max(srt.nworld, 1), NV = (size_t)vbeg[nhulls], NF = (size_t)fbeg[nhulls],
                 NE = (size_t)ebeg[nhulls];
    FbrBlob blob;
    const size_t ocen = blob.add<double>(nr * 3), odiam = blob.add<double>(diam.begin(), diam.begin() + nhulls), oworld = blob.add<double>(nw * 12);
    const size_t overts = blob.add<double>(verts, verts + NV * 3), oplanes = blob.add<double>(planes, planes + NF * 4);
    const size_t osteps = blob.add<int>(prog.steps.begin(), prog.steps.end()), obeg = blob.add<int>(srt.beg.begin(), srt.beg.end());
    const size_t oid = blob.add<int>(srt.id.begin(), srt.id.end()), otab = blob.add<int>((size_t)nhulls * 8), oedges = blob.add<int>(edges, edges + NE * 4);
    const size_t opairs = blob.add<int>(2 * (size_t)std::max(npairs, 1), sizeof(int2));
    for (int h = 0; h < nhulls; h++) {
        int *tb = blob.at<int>(otab) + (size_t)h * 8;
        tb[0] = srt.code[h], tb[1] = vbeg[h], tb[2] = vbeg[h + 1] - vbeg[h], tb[3] = fbeg[h], tb[4] = fbeg[h + 1] - fbeg[h], tb[5] = ebeg[h],
        tb[6] = ebeg[h + 1] - ebeg[h];
        if (link[h] >= 0) {
            std::copy(offset + 3 * h, offset + 3 * h + 3, blob.at<double>(ocen) + (size_t)srt.slot[h] * 3);
        } else {
            double *w = blob.at<double>(oworld) + (size_t)(-1 - srt.code[h]) * 12;
            std::copy(rot + 9 * h, rot + 9 * h + 9, w);
            std::copy(offset + 3 * h, offset + 3 * h + 3, w + 9);
        }
    }
    std::copy(pairs, pairs + 2 * (size_t)npairs, blob.at<int>(opairs));
    if (int rc = upload_blob(m->hs.set_tab, blob)) return rc;
    const char *base = (const char *)m->hs.set_tab.p;
    DevHulls dh;
    dh.fr = DevBoxes{prog.nsteps, prog.nslots, srt.nrob, 0, 0, offset_in_link_axes ? 1 : 0, (const int *)(base + osteps), (const int *)(base + obeg),
                     (const int *)(base + oid), (const double *)(base + ocen), nullptr, nullptr, nullptr};
    dh.nhulls = nhulls;
    dh.npairs = npairs;
    dh.tab = (const int *)(base + otab);
    dh.diam = (const double *)(base + odiam);
    dh.world = (const double *)(base + oworld);
    dh.verts = (const double *)(base + overts);
    dh.planes = (const double *)(base + oplanes);
    dh.edges = (const int *)(base + oedges);
    dh.pairs = (const int2 *)(base + opairs);
    dh.col = nullptr;
    dh.ldp = npairs;
    DevPairGrad dg;
    if (int rc = upload_grad_table(m->hs.grad_tab, srt, link, npairs, pairs, &dg)) return rc;
    FbrHullSet::Host hh;
    hh.link.assign(link, link + nhulls);
    hh.vbeg.assign(vbeg, vbeg + nhulls + 1);
    hh.fbeg.assign(fbeg, fbeg + nhulls + 1);
    hh.pairs.assign(pairs, pairs + 2 * (size_t)npairs);
    hh.verts.assign(verts, verts + NV * 3);
    hh.planes.assign(planes, planes + NF * 4);
    hh.diam.assign(diam.begin(), diam.begin() + nhulls);
    FbrHullViews views;
    if (int rc = build_hull_views(m, dh, hh, large, nullptr, FBR_MESHES_NONE, views)) return rc;
    int big = -1;
    for (int h = 0; h < nhulls && big < 0; h++)
        if (vbeg[h + 1] - vbeg[h] > FBR_MAX_HULL_VERTICES) big = h;
    m->hs.set = dh;
    m->hs.grad = dg;
    m->hs.host = std::move(hh);
    m->hs.large_set = large;
    m->hs.big = big;
    m->hs.big_nv = big < 0 ? 0 : vbeg[big + 1] - vbeg[big];
    m->hs.views = std::move(views);
    return FBR_OK;
}

extern "C" int fbr_model_set_hulls(fbr_model *m, int32_t nhulls, const int32_t *link, const double *offset, const double *rot,
                                   int32_t offset_in_link_axes, const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes,
                                   const int32_t *ebeg, const int32_t *edges, int32_t npairs, const int32_t *pairs)
{
    return install_hulls(m, FBR_MAX_HULL_VERTICES, false, nhulls, link, offset, rot, offset_in_link_axes, vbeg, verts, fbeg, planes, ebeg, edges, npairs, pairs);
}

extern "C" int fbr_model_set_large_hulls(fbr_model *m, int32_t nhulls, const int32_t *link, const double *offset, const double *rot,
                                         int32_t offset_in_link_axes, const int32_t *vbeg, const double *verts, const int32_t *fbeg,
                                         const double *planes, const int32_t *ebeg, const int32_t *edges, int32_t npairs, const int32_t *pairs)
{
    return install_hulls(m, FBR_MAX_LARGE_HULL_VERTICES, true, nhulls, link, offset, rot, offset_in_link_axes, vbeg, verts, fbeg, planes, ebeg, edges, npairs,
                         pairs);
}

// the hull set has a hull above FBR_MAX_HULL_VERTICES vertices: what `who` does is not built for it
static bool refuse_large_hulls(const fbr_model *m, const char *who)
{
    if (m->hs.big < 0) return false;
    set_err(std::string(who) + ": hull " + std::to_string(m->hs.big) + " of the set has " + std::to_string(m->hs.big_nv) + " vertices, more than " +
            std::to_string(FBR_MAX_HULL_VERTICES) + " (a set of fbr_model_set_large_hulls: distances only, no meshes and no gradients)");
    return true;
}

// ---- triangle meshes on hulls of the set (csrc/fbr_mesh.h) ---------------------------------------------------------------------------------
// fbr_model_set_hull_meshes (large false: the caps of the brute-force kernel, small hulls only) and fbr_model_set_large_hull_meshes (large:
// the cap of the trees of csrc/fbr_mesh_bvh.h, no cap on a pair's work, any hull set): one attachment, two kernels
static int attach_meshes(fbr_model *m, bool large, int32_t nmesh, const int32_t *hull, const int32_t *tbeg, const double *tris)
{
    if (!m) {
        set_err("null model");
        return FBR_E_INVALID;
    }
    if (!large && refuse_large_hulls(m, "fbr_model_set_hull_meshes")) return FBR_E_INVALID;
    FbrHullSet &H = m->hs;
    const auto &hh = H.host;
    const int nhulls = H.set.nhulls, npairs = H.set.npairs;
    const std::string bad = fbr_mesh_validate(nhulls, hh.link.data(), hh.fbeg.data(), hh.planes.data(), hh.diam.data(), npairs, hh.pairs.data(),
                                              large ? FBR_MAX_LARGE_MESH_TRIANGLES : FBR_MAX_MESH_TRIANGLES,
                                              large ? std::numeric_limits<long>::max() : (long)FBR_MAX_MESH_PAIR_WORK, nmesh, hull, tbeg, tris);
    if (!bad.empty()) {
        set_err(bad);
        return FBR_E_INVALID;
    }
    // the trees, and the triangles in their order: what the tables below hold of a large attachment
    FbrMeshBvhSet bvh;
    if (large && nmesh > 0) {
        const std::string deep = fbr_mesh_bvh_set(nmesh, tbeg, tris, bvh);
        if (!deep.empty()) {
            set_err("hull meshes: " + deep);
            return FBR_E_INVALID;
        }
        tris = bvh.tris.data();
    }
    if (int rc = enter_blocking(m)) return rc;  // (no launch that reads the tables replaced below is in flight)
    HIPCHK(hipStreamSynchronize(m->stream));
    // Unlike the three setters above, which reuse their buffers (they have cleared their set before they build), this one builds into fresh
    // allocations and swaps them in once the copies have succeeded: a call that fails here leaves the attachments in place as well.
    FbrHullViews views;
    if (nmesh == 0) {
        if (int rc = build_hull_views(m, H.set, hh, H.large_set, nullptr, FBR_MESHES_NONE, views)) return rc;
        H.clear_meshes();
        H.views = std::move(views);
        return FBR_OK;
    }
    std::vector<int> mtab((size_t)nhulls * 2, 0);
    for (int i = 0; i < nmesh; i++) mtab[2 * (size_t)hull[i]] = tbeg[i], mtab[2 * (size_t)hull[i] + 1] = tbeg[i + 1] - tbeg[i];
    const int kind = large ? FBR_MESHES_TREE : FBR_MESHES_SMALL;
    if (int rc = build_hull_views(m, H.set, hh, H.large_set, mtab.data(), kind, views)) return rc;
    // one allocation: sph | tris | aux | mtab | first node of a hull's tree | nodes | node spheres (the last three: a large attachment)
    const size_t NT = (size_t)tbeg[nmesh];
    FbrBlob blob;
    const size_t osph = blob.add<double>((size_t)nhulls * 4), otris = blob.add<double>(tris, tris + NT * 9), oaux = blob.add<double>(NT * 5);
    const size_t ovol = blob.add<double>(bvh.vol.begin(), bvh.vol.end()), omtab = blob.add<int>(mtab.begin(), mtab.end());
    const size_t onbeg = blob.add<int>((size_t)nhulls), onode = blob.add<int>(bvh.node.begin(), bvh.node.end());
    if (large)
        for (int i = 0; i < nmesh; i++) blob.at<int>(onbeg)[hull[i]] = bvh.nbeg[i];
    for (int h = 0; h < nhulls; h++)
        fbr_mesh_point_sphere(hh.vbeg[h + 1] - hh.vbeg[h], hh.verts.data() + 3 * (size_t)hh.vbeg[h], 3L * mtab[2 * (size_t)h + 1],
                              tris + 9 * (size_t)mtab[2 * (size_t)h], blob.at<double>(osph) + 4 * (size_t)h);
    for (size_t t = 0; t < NT; t++) fbr_mesh_triangle_aux(tris + 9 * t, blob.at<double>(oaux) + 5 * t);  // (large: what bvh.aux holds)
    DevBuf fresh;
    if (int rc = upload_blob(fresh, blob)) return rc;
    H.mesh_tab = std::move(fresh);
    H.views = std::move(views);
    const char *base = (const char *)H.mesh_tab.p;
    H.geo = DevMeshes{0, (const int *)(base + omtab), (const double *)(base + osph), (const double *)(base + otris), (const double *)(base + oaux),
                      nullptr, nullptr};
    H.bvh = DevMeshBvh{(const int *)(base + onbeg), (const int *)(base + onode), (const double *)(base + ovol)};
    H.meshes = kind;
    return FBR_OK;
}

extern "C" int fbr_model_set_hull_meshes(fbr_model *m, int32_t nmesh, const int32_t *hull, const int32_t *tbeg, const double *tris)
{
    return attach_meshes(m, false, nmesh, hull, tbeg, tris);
}

extern "C" int fbr_model_set_large_hull_meshes(fbr_model *m, int32_t nmesh, const int32_t *hull, const int32_t *tbeg, const double *tris)
{
    return attach_meshes(m, true, nmesh, hull, tbeg, tris);
}

// attachments of fbr_model_set_large_hull_meshes are in place: `who` has no gradients of them (fbr_large_mesh_distance_gradients has; the
// message is the one from before that call existed: callers match it)
static bool refuse_large_meshes(const fbr_model *m, const char *who)
{
    if (m->hs.meshes != FBR_MESHES_TREE) return false;
    set_err(std::string(who) + ": the hull set has triangle meshes attached by fbr_model_set_large_hull_meshes: distances only "
                               "(fbr_candidate_hull_distances), gradients of such a set are not built");
    return true;
}

// ---- candidate distances -------------------------------------------------------------------------------------------------------------
// The capsule, the box and the hull call share everything but what walks the tree and what measures the pairs.  missing: the message when
// there is no set (null: there is one); walk_kernel, walk_blk, walk_buf: the kernel that writes a block's world endpoints or frames, the
// bytes of a block of its output and the workspace that holds them; nslots the branch points of the set's program; P the pairs, nbatch the
// batches of pairs a block of samples is cut into, pairs_cap the waves per CU the pairs grid stops at;
// launch_walk(grid, lds, tl, b0, nb, stage, ldn, q, rpy, bpos, out, scratch) and launch_pairs(grid, tl, b0, nb, out, pval, pidx) the kernels.
template <class LaunchWalk, class LaunchPairs>
static int candidate_distances(fbr_model *m, const char *missing, const void *walk_kernel, size_t walk_blk, DevBuf fbr_model::*walk_buf, int nslots, long P,
                               long nbatch, int pairs_cap, const fbr_states *st, const double *base_pos, int32_t ncand, int32_t step, double *dist_out,
                               int64_t *idx_out, int32_t out_mem, LaunchWalk launch_walk, LaunchPairs launch_pairs)
{
    if (!m || !st || !dist_out || !idx_out) {
        set_err("null model / states / dist_out / idx_out");
        return FBR_E_INVALID;
    }
    if (st->num_samples < 0 || (st->mem != FBR_HOST && st->mem != FBR_DEVICE) || !st->q) {
        set_err("bad fbr_states header, or q is NULL");
        return FBR_E_INVALID;
    }
    if (missing) {
        set_err(missing);
        return FBR_E_INVALID;
    }
    if (ncand < 1 || step < 1) {
        set_err("ncand and step must be at least 1");
        return FBR_E_INVALID;
    }
    if (st->num_samples <= 0 || st->num_samples % ncand != 0) {
        set_err("num_samples must be a positive multiple of ncand (equal candidates of consecutive samples)");
        return FBR_E_INVALID;
    }
    if (int rc = enter_blocking(m)) return rc;
    const FbrHostModel &hm = m->hm;
    const long S = st->num_samples, C = ncand;
    const double *dq = nullptr, *drpy = nullptr, *dbp = nullptr;
    int rc;
    if ((rc = stage_one(m, m->st_q, st->q, (size_t)S * hm.n, st->mem, &dq))) return rc;
    if (hm.floating && st->base_rpy) {
        if ((rc = stage_one(m, m->st_rpy, st->base_rpy, (size_t)S * 3, st->mem, &drpy))) return rc;
        if ((rc = stage_one(m, m->st_bpos, base_pos, (size_t)S * 3, st->mem, &dbp))) return rc;
    }
    DevCapTiles tl;
    tl.T = S / C;
    tl.step = step;
    tl.Tc = (tl.T + step - 1) / step;
    tl.tiles = (tl.Tc + 63) / 64;
    tl.nblk = C * tl.tiles;
    // blocks per launch: the walk's output of the blocks in flight stays below 256 MB, their partials below 64 MB
    const size_t part_blk = (size_t)P * (sizeof(double) + sizeof(long));
    long ch = (long)std::min((size_t)(256u << 20) / walk_blk, (size_t)(64u << 20) / part_blk);
    if (m->opt.chunk_samples >= 1) ch = (long)m->opt.chunk_samples / 64;  // (tests: the multi-launch path at small sizes)
    ch = std::max(1L, std::min(ch, tl.nblk));
    DevBuf &wbuf = m->*walk_buf;
    if ((rc = wbuf.ensure((size_t)ch * walk_blk))) return rc;
    if ((rc = m->cap_part.ensure((size_t)ch * part_blk))) return rc;
    double *pval = m->cap_part.as<double>();
    long *pidx = (long *)(pval + (size_t)ch * P);
    const size_t cnt = (size_t)C * P;
    double *val = dist_out;
    long *idx = (long *)idx_out;
    if (out_mem == FBR_HOST) {
        if ((rc = m->cap_out.ensure(cnt * (sizeof(double) + sizeof(long))))) return rc;
        val = m->cap_out.as<double>();
        idx = (long *)(val + cnt);
    }
    const int ldn = std::max(hm.n, 1) | 1;
    const size_t lds_want = (size_t)64 * ldn * sizeof(double);
    const int stage = lds_want <= (size_t)64 * 1024;  // up to 127 DOF; beyond, the lanes read their rows from memory
    const size_t lds = stage ? lds_want : 0;
    const int pgrid = (int)std::min<long>(ch, (long)m->num_cus * 8);
    if ((rc = m->cap_scratch.ensure((size_t)pgrid * std::max(nslots, 1) * 12 * 64 * sizeof(double)))) return rc;
    if (lds) HIPCHK(hipFuncSetAttribute(walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (long b0 = 0; b0 < tl.nblk; b0 += ch) {
        const long nb = std::min(ch, tl.nblk - b0);
        {
            ProfScope ps(m, FBR_PROF_KIN);
            launch_walk((unsigned)std::min<long>(nb, pgrid), lds, tl, b0, nb, stage, ldn, dq, drpy, dbp, wbuf.as<double>(), m->cap_scratch.as<double>());
            HIPCHK(hipGetLastError());
        }
        {
            ProfScope ps(m, FBR_PROF_REDUCE);
            launch_pairs((unsigned)std::min<long>(nb * nbatch, (long)m->num_cus * pairs_cap), tl, b0, nb, (const double *)wbuf.as<double>(), pval, pidx);
            HIPCHK(hipGetLastError());
            const long cands = (b0 + nb - 1) / tl.tiles - b0 / tl.tiles + 1;
            hipLaunchKernelGGL(fbr_capsule_finish_kernel, dim3((unsigned)((cands * P + 255) / 256)), dim3(256), 0, m->stream, tl, (int)P, b0, nb,
                               (const double *)pval, (const long *)pidx, val, idx);
            HIPCHK(hipGetLastError());
        }
    }
    if (out_mem == FBR_HOST) {
        HIPCHK(hipMemcpyAsync(dist_out, val, cnt * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(idx_out, idx, cnt * sizeof(long), hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    prof_collect(m);
    return FBR_OK;
}

extern "C" int fbr_candidate_capsule_distances(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, int32_t step,
                                               double *dist_out, int64_t *idx_out, int32_t out_mem)
{
    const bool have = m && m->caps.ncaps != 0 && m->caps.npairs != 0;
    const long P = m ? m->caps.npairs : 0, ncaps = m ? m->caps.ncaps : 0;
    return candidate_distances(
        m, !m || have ? nullptr : "no capsule set with at least one pair (fbr_model_set_capsules)", (const void *)fbr_capsule_points_kernel,
        (size_t)ncaps * 6 * 64 * sizeof(double), &fbr_model::cap_ep, m ? m->caps.nslots : 0, P, (P + FBR_CAPSULE_BATCH - 1) / FBR_CAPSULE_BATCH, 16, st,
        base_pos, ncand, step, dist_out, idx_out, out_mem,
        [&](unsigned grid, size_t lds, const DevCapTiles &tl, long b0, long nb, int stage, int ldn, const double *dq, const double *drpy, const double *dbp,
            double *ep, double *scratch) {
            hipLaunchKernelGGL(fbr_capsule_points_kernel, dim3(grid), dim3(64), lds, m->stream, m->dm, m->caps, tl, b0, nb, stage, ldn, dq, drpy, dbp, ep,
                               scratch);
        },
        [&](unsigned grid, const DevCapTiles &tl, long b0, long nb, const double *ep, double *pval, long *pidx) {
            hipLaunchKernelGGL(fbr_capsule_pairs_kernel, dim3(grid), dim3(64), 0, m->stream, m->caps, tl, b0, nb, ep, pval, pidx);
        });
}

// The box and the hull call walk the tree with the same kernel (for the hulls: on the DevBoxes view of the set) into the same workspace.
template <class LaunchPairs>
static int candidate_frame_distances(fbr_model *m, const char *missing, const DevBoxes &bx, long P, long nbatch, const fbr_states *st,
                                     const double *base_pos, int32_t ncand, int32_t step, double *dist_out, int64_t *idx_out, int32_t out_mem,
                                     LaunchPairs launch_pairs)
{
    return candidate_distances(
        m, missing, (const void *)fbr_box_frames_kernel, (size_t)bx.nrob * 12 * 64 * sizeof(double), &fbr_model::box_fr, bx.nslots, P, nbatch, 32, st, base_pos,
        ncand, step, dist_out, idx_out, out_mem,
        [&](unsigned grid, size_t lds, const DevCapTiles &tl, long b0, long nb, int stage, int ldn, const double *dq, const double *drpy, const double *dbp,
            double *fr, double *scratch) {
            hipLaunchKernelGGL(fbr_box_frames_kernel, dim3(grid), dim3(64), lds, m->stream, m->dm, bx, tl, b0, nb, stage, ldn, dq, drpy, dbp, fr, scratch);
        },
        launch_pairs);
}

extern "C" int fbr_candidate_box_distances(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, int32_t step, double *dist_out,
                                           int64_t *idx_out, int32_t out_mem)
{
    const bool have = m && m->boxes.nrob != 0 && m->boxes.npairs != 0;
    const DevBoxes &bx = m ? m->boxes : kNoBoxes;
    return candidate_frame_distances(m, !m || have ? nullptr : "no box set with at least one pair (fbr_model_set_boxes)", bx, bx.npairs,
                                     (bx.npairs + FBR_BOX_BATCH - 1) / FBR_BOX_BATCH, st, base_pos, ncand, step, dist_out, idx_out, out_mem,
                                     [&](unsigned grid, const DevCapTiles &tl, long b0, long nb, const double *fr, double *pval, long *pidx) {
                                         hipLaunchKernelGGL(fbr_box_pairs_kernel, dim3(grid), dim3(64), 0, m->stream, bx, tl, b0, nb, fr, pval, pidx);
                                     });
}

extern "C" int fbr_candidate_hull_distances(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, int32_t step, double *dist_out,
                                            int64_t *idx_out, int32_t out_mem)
{
    // (a set of world hulls only has no pairs: two world hulls are never paired)
    const bool have = m && m->hs.set.nhulls != 0 && m->hs.set.npairs != 0;
    const long P = m ? m->hs.set.npairs : 0;
    return candidate_frame_distances(
        m, !m || have ? nullptr : "no hull set with at least one pair (fbr_model_set_hulls)", m ? m->hs.set.fr : kNoBoxes, P,
        (P + FBR_HULL_BATCH - 1) / FBR_HULL_BATCH, st, base_pos, ncand, step, dist_out, idx_out, out_mem,
        [&](unsigned, const DevCapTiles &tl, long b0, long nb, const double *fr, double *pval, long *pidx) {
            const FbrHullSet &H = m->hs;
            // the pairs of a class (sets...: the view, or the whole set and what the mesh kernels take besides) on `kernel`, `batch` pairs an
            // item, into their own columns; a class without a pair launches nothing
            const auto launch = [&](long pairs, int batch, auto kernel, auto... sets) {
                if (pairs == 0) return;
                hipLaunchKernelGGL(kernel, dim3((unsigned)std::min(nb * ((pairs + batch - 1) / batch), (long)m->num_cus * 32)), dim3(64), 0, m->stream,
                                   sets..., tl, b0, nb, fr, pval, pidx);
            };
            // class   kernel
            // SMALL   fbr_hull_pairs_kernel -- fbr_hull_large_pairs_kernel on a set of fbr_model_set_large_hulls with option hull_large_all
            //         (not beside small meshes: DESIGN.md)
            // BIG     fbr_hull_large_pairs_kernel
            // MESH    fbr_mesh_pairs_kernel (small meshes), fbr_mesh_bvh_pairs_kernel (tree meshes)
            const bool all = H.large_set && m->opt.hull_large_all != 0 && H.meshes != FBR_MESHES_SMALL;
            if (all && H.meshes == FBR_MESHES_NONE) return launch(P, FBR_HULL_LARGE_BATCH, fbr_hull_large_pairs_kernel, H.set);  // (one launch)
            const DevHulls small = H.of(FBR_PAIR_SMALL), big = H.of(FBR_PAIR_BIG);
            const DevMeshes ms = H.mesh_pairs();
            if (all)
                launch(small.npairs, FBR_HULL_LARGE_BATCH, fbr_hull_large_pairs_kernel, small);
            else
                launch(small.npairs, FBR_HULL_BATCH, fbr_hull_pairs_kernel, small);
            launch(big.npairs, FBR_HULL_LARGE_BATCH, fbr_hull_large_pairs_kernel, big);
            if (H.meshes == FBR_MESHES_TREE)
                launch(ms.npairs, 1, fbr_mesh_bvh_pairs_kernel, H.set, ms, H.bvh);
            else
                launch(ms.npairs, FBR_MESH_BATCH, fbr_mesh_pairs_kernel, H.set, ms);
        });
}

// ---- distance and its joint-position gradient at chosen configurations (csrc/fbr_capsule_grad.h, fbr_box_grad.h, fbr_hull_grad.h,
// fbr_mesh_grad.h) ----
// The capsule, the box, the hull and the mesh call share everything but the set and the kernel: `name` the entry point, P / nslots the pairs and
// the branch points of its set, launch(grid, C, T, q, rpy, bpos, sample, scale, pose, dist, grad) the kernel -- or the kernels of the mesh
// call; it returns FBR_OK, or the code of a workspace it could not get.
template <class Launch>
static int distance_gradients(fbr_model *m, const char *name, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                              const double *scale, const int64_t *pose_sample, double *dist_out, double *grad_q_out, int32_t out_mem, long P, int nslots,
                              Launch launch)
{
    if (ncand < 1) {
        set_err("ncand must be at least 1");
        return FBR_E_INVALID;
    }
    if (st->num_samples <= 0 || st->num_samples % ncand != 0) {
        set_err("num_samples must be a positive multiple of ncand (equal candidates of consecutive samples)");
        return FBR_E_INVALID;
    }
    if (int rc = enter_blocking(m)) return rc;
    const FbrHostModel &hm = m->hm;
    const long S = st->num_samples, C = ncand, T = S / C;
    const size_t items = (size_t)C * P;
    const double *dq = nullptr, *drpy = nullptr, *dbp = nullptr, *dsmp = nullptr, *dscale = nullptr, *dpose = nullptr;
    int rc;
    if ((rc = stage_one(m, m->st_q, st->q, (size_t)S * hm.n, st->mem, &dq))) return rc;
    if (hm.floating && st->base_rpy) {
        if ((rc = stage_one(m, m->st_rpy, st->base_rpy, (size_t)S * 3, st->mem, &drpy))) return rc;
        if ((rc = stage_one(m, m->st_bpos, base_pos, (size_t)S * 3, st->mem, &dbp))) return rc;
    }
    // (the index arrays are 8 bytes an entry, like the doubles the staging helper copies)
    if ((rc = stage_one(m, m->st_dq, (const double *)sample, items, st->mem, &dsmp))) return rc;
    if ((rc = stage_one(m, m->st_ddq, (const double *)pose_sample, items, st->mem, &dpose))) return rc;
    if ((rc = stage_one(m, m->st_aux, scale, items, st->mem, &dscale))) return rc;
    double *ddist = dist_out, *dgrad = grad_q_out;
    if (out_mem == FBR_HOST) {
        if ((rc = m->cap_out.ensure(items * (1 + (size_t)hm.n) * sizeof(double)))) return rc;
        ddist = m->cap_out.as<double>();
        dgrad = ddist + items;
    }
    const long tiles = (C + 63) / 64;
    const int grid = (int)std::min<long>(P * tiles, (long)m->num_cus * 8);
    if ((rc = m->cap_scratch.ensure((size_t)grid * std::max(nslots, 1) * 12 * 64 * sizeof(double)))) return rc;
    if ((rc = m->capg_flag.ensure(sizeof(int)))) return rc;
    int flag = 0;
    HIPCHK(hipMemsetAsync(m->capg_flag.p, 0, sizeof(int), m->stream));
    HIPCHK(hipMemsetAsync(dgrad, 0, items * hm.n * sizeof(double), m->stream));  // (joints off a pair's path: exact zeros, never touched by the kernel)
    {
        ProfScope ps(m, FBR_PROF_KIN);
        if ((rc = launch(grid, C, T, dq, drpy, dbp, (const long *)dsmp, dscale, (const long *)dpose, ddist, dgrad))) return rc;
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(&flag, m->capg_flag.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    if (out_mem == FBR_HOST) {
        HIPCHK(hipMemcpyAsync(dist_out, ddist, items * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(grad_q_out, dgrad, items * hm.n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    prof_collect(m);
    if (flag) {
        set_err(std::string(name) + ": a sample or pose_sample index lies outside -1 .. T - 1");
        return FBR_E_INVALID;
    }
    return FBR_OK;
}

static bool distance_gradient_args(const fbr_model *m, const fbr_states *st, const int64_t *sample, const double *dist_out, const double *grad_q_out,
                                   int32_t out_mem)
{
    if (!m || !st || !sample || !dist_out || !grad_q_out) {
        set_err("null model / states / sample / dist_out / grad_q_out");
        return false;
    }
    if (st->num_samples < 0 || (st->mem != FBR_HOST && st->mem != FBR_DEVICE) || !st->q || (out_mem != FBR_HOST && out_mem != FBR_DEVICE)) {
        set_err("bad fbr_states header or memory space, or q is NULL");
        return false;
    }
    return true;
}

extern "C" int fbr_capsule_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                              const double *scale, const int64_t *pose_sample, double *dist_out, double *grad_q_out, int32_t out_mem)
{
    if (!distance_gradient_args(m, st, sample, dist_out, grad_q_out, out_mem)) return FBR_E_INVALID;
    if (m->caps.ncaps == 0 || m->caps.npairs == 0) {
        set_err("no capsule set with at least one pair (fbr_model_set_capsules)");
        return FBR_E_INVALID;
    }
    return distance_gradients(m, "fbr_capsule_distance_gradients", st, base_pos, ncand, sample, scale, pose_sample, dist_out, grad_q_out, out_mem,
                              m->caps.npairs, m->caps.nslots,
                              [&](int grid, long C, long T, const double *dq, const double *drpy, const double *dbp, const long *dsmp, const double *dscale,
                                  const long *dpose, double *ddist, double *dgrad) {
                                  hipLaunchKernelGGL(fbr_capsule_grad_kernel, dim3((unsigned)grid), dim3(64), 0, m->stream, m->dm, m->caps, m->capg, C, T, dq,
                                                     drpy, dbp, dsmp, dscale, dpose, ddist, dgrad, m->cap_scratch.as<double>(), m->capg_flag.as<int>());
                                  return FBR_OK;
                              });
}

extern "C" int fbr_box_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                          const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out, double *grad_q_out,
                                          int32_t out_mem)
{
    if (!distance_gradient_args(m, st, sample, dist_out, grad_q_out, out_mem)) return FBR_E_INVALID;
    if (!std::isfinite(epsilon) || !(epsilon > 0.0)) {
        set_err("epsilon must be finite and positive");
        return FBR_E_INVALID;
    }
    if (m->boxes.nrob == 0 || m->boxes.npairs == 0) {
        set_err("no box set with at least one pair (fbr_model_set_boxes)");
        return FBR_E_INVALID;
    }
    double se, omc;
    fbr_boxgrad_trig(epsilon, &se, &omc);
    return distance_gradients(m, "fbr_box_distance_gradients", st, base_pos, ncand, sample, scale, pose_sample, dist_out, grad_q_out, out_mem,
                              m->boxes.npairs, m->boxes.nslots,
                              [&](int grid, long C, long T, const double *dq, const double *drpy, const double *dbp, const long *dsmp, const double *dscale,
                                  const long *dpose, double *ddist, double *dgrad) {
                                  hipLaunchKernelGGL(fbr_box_grad_kernel, dim3((unsigned)grid), dim3(64), 0, m->stream, m->dm, m->boxes, m->boxg, C, T, dq, drpy,
                                                     dbp, dsmp, dscale, dpose, epsilon, se, omc, ddist, dgrad, m->cap_scratch.as<double>(),
                                                     m->capg_flag.as<int>());
                                  return FBR_OK;
                              });
}

extern "C" int fbr_hull_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                           const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out, double *grad_q_out,
                                           int32_t out_mem)
{
    if (!distance_gradient_args(m, st, sample, dist_out, grad_q_out, out_mem)) return FBR_E_INVALID;
    if (!std::isfinite(epsilon) || !(epsilon > 0.0)) {
        set_err("epsilon must be finite and positive");
        return FBR_E_INVALID;
    }
    if (m->hs.set.nhulls == 0 || m->hs.set.npairs == 0) {
        set_err("no hull set with at least one pair (fbr_model_set_hulls)");
        return FBR_E_INVALID;
    }
    if (refuse_large_meshes(m, "fbr_hull_distance_gradients")) return FBR_E_UNSUPPORTED;
    if (refuse_large_hulls(m, "fbr_hull_distance_gradients")) return FBR_E_INVALID;
    if (m->hs.meshes != FBR_MESHES_NONE) {
        set_err("fbr_hull_distance_gradients: the hull set has triangle meshes attached (fbr_model_set_hull_meshes); gradients of mesh pairs are not built");
        return FBR_E_UNSUPPORTED;
    }
    double se, omc;
    fbr_boxgrad_trig(epsilon, &se, &omc);
    return distance_gradients(m, "fbr_hull_distance_gradients", st, base_pos, ncand, sample, scale, pose_sample, dist_out, grad_q_out, out_mem,
                              m->hs.set.npairs, m->hs.set.fr.nslots,
                              [&](int grid, long C, long T, const double *dq, const double *drpy, const double *dbp, const long *dsmp, const double *dscale,
                                  const long *dpose, double *ddist, double *dgrad) {
                                  hipLaunchKernelGGL(fbr_hull_grad_kernel, dim3((unsigned)grid), dim3(64), 0, m->stream, m->dm, m->hs.set, m->hs.grad, C, T, dq,
                                                     drpy, dbp, dsmp, dscale, dpose, epsilon, se, omc, ddist, dgrad, m->cap_scratch.as<double>(),
                                                     m->capg_flag.as<int>());
                                  return FBR_OK;
                              });
}

// The staged gradient calls: the pairs of `small` through fbr_hull_grad_kernel, into their columns; every class of `staged` -- pl pairs of a
// view, sg its stencil table -- through three stages (csrc/fbr_mesh_grad.h): A(grid, C, T, q, rpy, bpos, sample, scale, pose, se, omc, rel)
// records the relative pose of every stencil point, B(C, tiles, rel, dv) measures them, Q(grid, C, T, sample, pose, dv, dist, grad) forms
// the quotients.  The stages' kernels are each class's own: as one kernel for two they missed the register and timing rule.
// The classes write disjoint columns, so their order does not matter to a value.
struct StagedClass {
    long pl;
    const FbrStencil *sg;
    std::function<void(unsigned, long, long, const double *, const double *, const double *, const long *, const double *, const long *, double, double,
                       double *)>
        A;
    std::function<void(long, long, const double *, double *)> B;
    std::function<void(unsigned, long, long, const long *, const long *, const double *, double *, double *)> Q;
};

static int staged_distance_gradients(fbr_model *m, const char *name, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                     const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out, double *grad_q_out,
                                     int32_t out_mem, const DevHulls &small, const std::vector<StagedClass> &staged)
{
    double se, omc;
    fbr_boxgrad_trig(epsilon, &se, &omc);
    const FbrHullSet &H = m->hs;
    return distance_gradients(
        m, name, st, base_pos, ncand, sample, scale, pose_sample, dist_out, grad_q_out, out_mem, H.set.npairs, H.set.fr.nslots,
        [&](int grid, long C, long T, const double *dq, const double *drpy, const double *dbp, const long *dsmp, const double *dscale, const long *dpose,
            double *ddist, double *dgrad) -> int {
            const long tiles = (C + 63) / 64, ps = small.npairs;
            if (ps > 0)
                hipLaunchKernelGGL(fbr_hull_grad_kernel, dim3((unsigned)std::min<long>(ps * tiles, grid)), dim3(64), 0, m->stream, m->dm, small, H.grad, C, T,
                                   dq, drpy, dbp, dsmp, dscale, dpose, epsilon, se, omc, ddist, dgrad, m->cap_scratch.as<double>(),
                                   m->capg_flag.as<int>());
            // per class the recorded poses [ni][13][C] | the stencil distances [ni][C], one class after the other
            size_t total = 0;
            for (const StagedClass &sc : staged) {
                if (sc.pl == 0) continue;
                if ((long)sc.sg->sbeg.size() != sc.pl + 1) {
                    set_err(std::string(name) + ": the stencil tables do not match the set");
                    return FBR_E_INVALID;
                }
                total += (size_t)sc.sg->dev.nitems * (FBR_MESHGRAD_REL + 1) * (size_t)C;
            }
            if (total == 0) return FBR_OK;
            if (int rc = m->hs.work.ensure(total * sizeof(double))) return rc;
            double *rel = m->hs.work.as<double>();
            for (const StagedClass &sc : staged) {
                if (sc.pl == 0) continue;
                const size_t ni = (size_t)sc.sg->dev.nitems;
                double *dv = rel + ni * FBR_MESHGRAD_REL * (size_t)C;
                sc.A((unsigned)std::min<long>(sc.pl * tiles, grid), C, T, dq, drpy, dbp, dsmp, dscale, dpose, se, omc, rel);
                {
                    ProfScope pb(m, FBR_PROF_REDUCE);  // (stage B by itself, inside the call's FBR_PROF_KIN)
                    sc.B(C, tiles, (const double *)rel, dv);
                }
                sc.Q((unsigned)((C * sc.pl + 255) / 256), C, T, dsmp, dpose, (const double *)dv, ddist, dgrad);
                rel = dv + ni * (size_t)C;
            }
            return FBR_OK;
        });
}

// the three launches of the BIG class (csrc/fbr_hull_large_grad.h) on the view `staged` with the stencil table sg; wopt: option hull_grad_tile
static StagedClass large_hull_class(fbr_model *m, const DevHulls &staged, const FbrStencil &sg, double epsilon, double wopt)
{
    const FbrHullSet &H = m->hs;
    const FbrStencil *psg = &sg;
    return StagedClass{
        staged.npairs, psg,
        [=, &H](unsigned grid, long C, long T, const double *dq, const double *drpy, const double *dbp, const long *dsmp, const double *dscale,
                const long *dpose, double se, double omc, double *rel) {
            hipLaunchKernelGGL(fbr_hull_large_grad_frames_kernel, dim3(grid), dim3(64), 0, m->stream, m->dm, staged, H.grad, psg->dev, C, T, dq, drpy, dbp, dsmp,
                               dscale, dpose, epsilon, se, omc, rel, m->cap_scratch.as<double>(), m->capg_flag.as<int>());
        },
        [=](long C, long, const double *rel, double *dv) {
            const long pl = staged.npairs;
            const int width =
                wopt != 0 ? (int)wopt : fbr_hull_large_grad_width(psg->sbeg.data(), (int)pl, C, (long)FBR_HULL_LARGE_GRAD_WAVES_PER_CU * m->num_cus);
            const long tpp = ((long)psg->dev.smax * C + width - 1) / width;
            hipLaunchKernelGGL(fbr_hull_large_grad_dist_kernel, dim3((unsigned)std::min<long>(pl * tpp, (long)m->num_cus * 32)), dim3(64), 0, m->stream, staged,
                               psg->dev, C, width, tpp, rel, dv);
        },
        [=](unsigned grid, long C, long T, const long *dsmp, const long *dpose, const double *dv, double *ddist, double *dgrad) {
            hipLaunchKernelGGL(fbr_hull_large_grad_quot_kernel, dim3(grid), dim3(256), 0, m->stream, staged, psg->dev, (int)m->hm.n, C, T, dsmp, dpose, epsilon,
                               dv, ddist, dgrad);
        }};
}

// the three launches of the MESH class: stages A and C of csrc/fbr_mesh_grad.h; stage B launch_B(ms, mg, C, tiles, rel, dv) the attachment's own
template <class LaunchB> static StagedClass mesh_class(fbr_model *m, double epsilon, LaunchB launch_B)
{
    const FbrHullSet &H = m->hs;
    const DevMeshes ms = H.mesh_pairs();
    const DevMeshGrad mg = H.views.mesh.dev;
    return StagedClass{
        ms.npairs, &H.views.mesh,
        [=, &H](unsigned grid, long C, long T, const double *dq, const double *drpy, const double *dbp, const long *dsmp, const double *dscale,
                const long *dpose, double se, double omc, double *rel) {
            hipLaunchKernelGGL(fbr_mesh_grad_frames_kernel, dim3(grid), dim3(64), 0, m->stream, m->dm, H.set, H.grad, ms, mg, C, T, dq, drpy, dbp, dsmp, dscale,
                               dpose, epsilon, se, omc, rel, m->cap_scratch.as<double>(), m->capg_flag.as<int>());
        },
        [=](long C, long tiles, const double *rel, double *dv) { launch_B(ms, mg, C, tiles, rel, dv); },
        [=, &H](unsigned grid, long C, long T, const long *dsmp, const long *dpose, const double *dv, double *ddist, double *dgrad) {
            hipLaunchKernelGGL(fbr_mesh_grad_quot_kernel, dim3(grid), dim3(256), 0, m->stream, H.set, ms, mg, (int)m->hm.n, C, T, dsmp, dpose, epsilon, dv,
                               ddist, dgrad);
        }};
}

// A hull set with triangle meshes attached (fbr_model_set_hull_meshes): the SMALL pairs directly, the MESH pairs staged.
extern "C" int fbr_mesh_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                           const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out, double *grad_q_out,
                                           int32_t out_mem)
{
    if (!distance_gradient_args(m, st, sample, dist_out, grad_q_out, out_mem)) return FBR_E_INVALID;
    if (!std::isfinite(epsilon) || !(epsilon > 0.0)) {
        set_err("epsilon must be finite and positive");
        return FBR_E_INVALID;
    }
    if (m->hs.set.nhulls == 0 || m->hs.set.npairs == 0) {
        set_err("no hull set with at least one pair (fbr_model_set_hulls)");
        return FBR_E_INVALID;
    }
    if (refuse_large_meshes(m, "fbr_mesh_distance_gradients")) return FBR_E_UNSUPPORTED;
    if (refuse_large_hulls(m, "fbr_mesh_distance_gradients")) return FBR_E_INVALID;
    if (m->hs.meshes == FBR_MESHES_NONE) {
        set_err("fbr_mesh_distance_gradients: the hull set has no triangle meshes attached (fbr_model_set_hull_meshes); fbr_hull_distance_gradients "
                "serves a set of hulls only");
        return FBR_E_INVALID;
    }
    const FbrHullSet &H = m->hs;
    return staged_distance_gradients(
        m, "fbr_mesh_distance_gradients", st, base_pos, ncand, sample, scale, pose_sample, epsilon, dist_out, grad_q_out, out_mem, H.of(FBR_PAIR_SMALL),
        {mesh_class(m, epsilon, [m, &H](const DevMeshes &ms, const DevMeshGrad &mg, long C, long tiles, const double *rel, double *dv) {
            hipLaunchKernelGGL(fbr_mesh_grad_dist_kernel, dim3((unsigned)std::min<long>(mg.nitems * tiles, (long)m->num_cus * 32)), dim3(64), 0, m->stream,
                               H.set, ms, mg, C, rel, dv);
        })});
}

// A hull set installed by fbr_model_set_large_hulls: the SMALL pairs directly, the BIG pairs -- every pair with option hull_large_all --
// staged (csrc/fbr_hull_large_grad.h).
extern "C" int fbr_large_hull_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                                 const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out,
                                                 double *grad_q_out, int32_t out_mem)
{
    if (!distance_gradient_args(m, st, sample, dist_out, grad_q_out, out_mem)) return FBR_E_INVALID;
    if (!std::isfinite(epsilon) || !(epsilon > 0.0)) {
        set_err("fbr_large_hull_distance_gradients: epsilon must be finite and positive");
        return FBR_E_INVALID;
    }
    if (m->hs.set.nhulls == 0 || !m->hs.large_set) {
        set_err("fbr_large_hull_distance_gradients: no hull set installed by fbr_model_set_large_hulls (fbr_hull_distance_gradients serves a set of "
                "fbr_model_set_hulls)");
        return FBR_E_INVALID;
    }
    if (m->hs.set.npairs == 0) {
        set_err("fbr_large_hull_distance_gradients: the hull set has no pair");
        return FBR_E_INVALID;
    }
    if (refuse_large_meshes(m, "fbr_large_hull_distance_gradients")) return FBR_E_UNSUPPORTED;
    if (m->hs.meshes != FBR_MESHES_NONE) {  // (fbr_model_set_hull_meshes: only a set without a hull above the cap can have them)
        set_err("fbr_large_hull_distance_gradients: the hull set has triangle meshes attached (fbr_model_set_hull_meshes); "
                "fbr_mesh_distance_gradients serves such a set");
        return FBR_E_UNSUPPORTED;
    }
    const double wopt = m->opt.hull_grad_tile;
    if (!(wopt == 0 || wopt == 1 || wopt == 2 || wopt == 4 || wopt == 8 || wopt == 16 || wopt == 32 || wopt == 64)) {
        set_err("fbr_large_hull_distance_gradients: option hull_grad_tile must be 0 or a power of two from 1 to 64");
        return FBR_E_INVALID;
    }
    const FbrHullSet &H = m->hs;
    const bool all = m->opt.hull_large_all != 0;
    const DevHulls small = all ? kNoHulls : H.of(FBR_PAIR_SMALL), staged = all ? H.set : H.of(FBR_PAIR_BIG);
    const FbrStencil &sg = all ? H.views.all : H.views.big;
    return staged_distance_gradients(m, "fbr_large_hull_distance_gradients", st, base_pos, ncand, sample, scale, pose_sample, epsilon, dist_out, grad_q_out,
                                     out_mem, small, {large_hull_class(m, staged, sg, epsilon, wopt)});
}

// A hull set of either setter with a tree attachment (fbr_model_set_large_hull_meshes): the SMALL pairs directly, the BIG pairs through the
// stages of csrc/fbr_hull_large_grad.h, the MESH pairs through stages A and C of csrc/fbr_mesh_grad.h around the tree stage of
// csrc/fbr_mesh_bvh_grad.h.  Option hull_large_all has no effect here.
extern "C" int fbr_large_mesh_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                                 const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out,
                                                 double *grad_q_out, int32_t out_mem)
{
    if (!distance_gradient_args(m, st, sample, dist_out, grad_q_out, out_mem)) return FBR_E_INVALID;
    if (!std::isfinite(epsilon) || !(epsilon > 0.0)) {
        set_err("fbr_large_mesh_distance_gradients: epsilon must be finite and positive");
        return FBR_E_INVALID;
    }
    if (m->hs.set.nhulls == 0 || m->hs.set.npairs == 0) {
        set_err("fbr_large_mesh_distance_gradients: no hull set with at least one pair (fbr_model_set_hulls, fbr_model_set_large_hulls)");
        return FBR_E_INVALID;
    }
    if (m->hs.meshes != FBR_MESHES_TREE) {
        set_err("fbr_large_mesh_distance_gradients: the hull set has no triangle meshes attached by fbr_model_set_large_hull_meshes; "
                "fbr_mesh_distance_gradients serves small meshes (fbr_model_set_hull_meshes), fbr_large_hull_distance_gradients large hulls without "
                "meshes (fbr_model_set_large_hulls), fbr_hull_distance_gradients small hulls without meshes (fbr_model_set_hulls)");
        return FBR_E_INVALID;
    }
    const double oopt = m->opt.mesh_grad_order;
    if (!(oopt == 0 || oopt == FBR_MESH_GRAD_CANDIDATE_MAJOR || oopt == FBR_MESH_GRAD_SLOT_MAJOR)) {
        set_err("fbr_large_mesh_distance_gradients: option mesh_grad_order must be 0 (the default order), 1 (candidate-major) or 2 (slot-major)");
        return FBR_E_INVALID;
    }
    const double wopt = m->opt.hull_grad_tile;  // (of the BIG class: not looked at by a set without such a pair)
    if (m->hs.of(FBR_PAIR_BIG).npairs > 0 && !(wopt == 0 || wopt == 1 || wopt == 2 || wopt == 4 || wopt == 8 || wopt == 16 || wopt == 32 || wopt == 64)) {
        set_err("fbr_large_mesh_distance_gradients: option hull_grad_tile must be 0 or a power of two from 1 to 64");
        return FBR_E_INVALID;
    }
    const int order = oopt == 0 ? FBR_MESH_GRAD_ORDER_DEFAULT : (int)oopt;
    const FbrHullSet &H = m->hs;
    return staged_distance_gradients(
        m, "fbr_large_mesh_distance_gradients", st, base_pos, ncand, sample, scale, pose_sample, epsilon, dist_out, grad_q_out, out_mem, H.of(FBR_PAIR_SMALL),
        {large_hull_class(m, H.of(FBR_PAIR_BIG), H.views.big, epsilon, wopt),
         mesh_class(m, epsilon, [m, &H, order](const DevMeshes &ms, const DevMeshGrad &mg, long C, long, const double *rel, double *dv) {
             const long tpp = ((long)mg.smax * C + 63) / 64;
             hipLaunchKernelGGL(fbr_mesh_bvh_grad_dist_kernel, dim3((unsigned)std::min<long>(ms.npairs * tpp, (long)m->num_cus * 32)), dim3(64), 0, m->stream,
                                H.set, ms, H.bvh, mg, C, order, tpp, rel, dv);
         })});
}
