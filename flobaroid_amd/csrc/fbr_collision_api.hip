// fbr_collision_api.hip -- the collision entry points of the C-ABI (include/fbr.h): the capsule, box and convex-hull sets, the triangle
// meshes attached to hulls, their candidate distances and their distance gradients.  The kernels are those of fbr_capsule.h, fbr_box.h,
// fbr_hull.h, fbr_mesh.h and their *_grad.h siblings (section FBR_KERNELS_COLLISION); the tables every set shares are built by
// fbr_collision_tables.h.  DESIGN.md, "collision layout".
#define FBR_KERNELS_COLLISION
#include "fbr_internal.h"
#include "fbr_collision_tables.h"
#include "fbr_hull_large_grad.h"
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

static const DevBoxes kNoBoxes = {0, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

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
    m->hulls = DevHulls{kNoBoxes, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    m->hullg = DevPairGrad{0, nullptr, nullptr};
    // (the meshes attached to the set before are gone with it: fbr_model_set_hull_meshes)
    m->hulls_plain = m->hulls;
    m->meshes = DevMeshes{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    m->meshg = DevMeshGrad{0, 0, nullptr, nullptr, nullptr};
    m->has_meshes = false;
    m->mesh_large = false;
    m->mesh_bvh = DevMeshBvh{nullptr, nullptr, nullptr};
    m->hulls_plain_big = m->hulls;
    m->hull_host = {};
    m->hulls_small = m->hulls_big = m->hulls;
    m->hull_big = -1;
    m->hull_big_nv = 0;
    m->hull_large_set = false;
    for (int i = 0; i < 2; i++) {
        m->hull_lgrad[i] = DevMeshGrad{0, 0, nullptr, nullptr, nullptr};
        m->hull_lgrad_sbeg[i].clear();
    }
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
    if (int rc = upload_blob(m->hull_tab, blob)) return rc;
    const char *base = (const char *)m->hull_tab.p;
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
    if (int rc = upload_grad_table(m->hullg_tab, srt, link, npairs, pairs, &m->hullg)) return rc;
    // a hull above the small cap: the pairs of two small hulls, in their order, and the others, in theirs, each with its columns
    int big = -1;
    for (int h = 0; h < nhulls && big < 0; h++)
        if (vbeg[h + 1] - vbeg[h] > FBR_MAX_HULL_VERTICES) big = h;
    DevHulls small = dh, rest = dh;
    if (big >= 0) {
        std::vector<int> sk, bk;
        for (int k = 0; k < npairs; k++) {
            const int a = pairs[2 * k], b = pairs[2 * k + 1];
            (vbeg[a + 1] - vbeg[a] > FBR_MAX_HULL_VERTICES || vbeg[b + 1] - vbeg[b] > FBR_MAX_HULL_VERTICES ? bk : sk).push_back(k);
        }
        const size_t ns = std::max(sk.size(), (size_t)1), nl = std::max(bk.size(), (size_t)1);
        FbrBlob split;  // small pairs | large pairs | small columns | large columns
        const size_t osp = split.add<int>(2 * ns, sizeof(int2)), olp = split.add<int>(2 * nl, sizeof(int2)), osc = split.add<int>(ns), olc = split.add<int>(nl);
        for (size_t i = 0; i < sk.size(); i++)
            split.at<int>(osp)[2 * i] = pairs[2 * sk[i]], split.at<int>(osp)[2 * i + 1] = pairs[2 * sk[i] + 1], split.at<int>(osc)[i] = sk[i];
        for (size_t i = 0; i < bk.size(); i++)
            split.at<int>(olp)[2 * i] = pairs[2 * bk[i]], split.at<int>(olp)[2 * i + 1] = pairs[2 * bk[i] + 1], split.at<int>(olc)[i] = bk[i];
        if (int rc = upload_blob(m->hull_split_tab, split)) return rc;
        const char *sb = (const char *)m->hull_split_tab.p;
        small.npairs = (int)sk.size(), small.pairs = (const int2 *)(sb + osp), small.col = (const int *)(sb + osc);
        rest.npairs = (int)bk.size(), rest.pairs = (const int2 *)(sb + olp), rest.col = (const int *)(sb + olc);
    }
    // the stencil points of fbr_large_hull_distance_gradients (csrc/fbr_hull_large_grad.h): per large pair the centre, then + eps, - eps of
    // every joint fbr_rigidgrad_item evaluates, in walk order -- for the pairs of `rest` and for every pair (option hull_large_all, read by
    // every call): sbeg | pair of a point | its joint, twice
    DevMeshGrad lgrad[2] = {{0, 0, nullptr, nullptr, nullptr}, {0, 0, nullptr, nullptr, nullptr}};
    std::vector<int> lsbeg[2];
    if (large && npairs > 0) {
        std::vector<int> stepof, anc, joint, gtab;
        fbr_capgrad_ancestors(hm, prog, stepof, anc);
        const auto isbig = [&](int h) { return vbeg[h + 1] - vbeg[h] > FBR_MAX_HULL_VERTICES; };
        size_t off[2], np[2];
        for (int arr = 0; arr < 2; arr++) {
            std::vector<int> gpair, gjoint;
            lsbeg[arr].assign(1, 0);
            int smax = 0;
            for (int k = 0; k < npairs; k++) {
                const int a = pairs[2 * k], b = pairs[2 * k + 1];
                if (arr == 0 && big >= 0 && !isbig(a) && !isbig(b)) continue;  // (no hull above the cap: `rest` is the whole set)
                fbr_meshgrad_slots(link[a] < 0 ? -1 : stepof[link[a]], link[b] < 0 ? -1 : stepof[link[b]], offset_in_link_axes ? 1 : 0, prog.steps.data(),
                                   anc.data(), fbr_capgrad_words(prog.nsteps), joint);
                gpair.insert(gpair.end(), joint.size(), (int)lsbeg[arr].size() - 1);
                gjoint.insert(gjoint.end(), joint.begin(), joint.end());
                lsbeg[arr].push_back(lsbeg[arr].back() + (int)joint.size());
                smax = std::max(smax, (int)joint.size());
            }
            off[arr] = gtab.size(), np[arr] = lsbeg[arr].size() - 1;
            lgrad[arr].nitems = (int)gpair.size(), lgrad[arr].smax = smax;
            gtab.insert(gtab.end(), lsbeg[arr].begin(), lsbeg[arr].end());
            gtab.insert(gtab.end(), gpair.begin(), gpair.end());
            gtab.insert(gtab.end(), gjoint.begin(), gjoint.end());
        }
        if (int rc = m->hull_lgrad_tab.ensure(gtab.size() * sizeof(int))) return rc;
        HIPCHK(hipMemcpy(m->hull_lgrad_tab.p, gtab.data(), gtab.size() * sizeof(int), hipMemcpyHostToDevice));
        for (int arr = 0; arr < 2; arr++) {
            const int *g = m->hull_lgrad_tab.as<int>() + off[arr];
            lgrad[arr].sbeg = g, lgrad[arr].spair = g + np[arr] + 1, lgrad[arr].sjoint = g + np[arr] + 1 + lgrad[arr].nitems;
        }
    }
    for (int i = 0; i < 2; i++) {
        m->hull_lgrad[i] = lgrad[i];
        m->hull_lgrad_sbeg[i] = lsbeg[i];
    }
    m->hulls = dh;
    m->hulls_plain = dh;
    m->hulls_small = small;
    m->hulls_big = rest;
    m->hull_big = big;
    m->hull_big_nv = big < 0 ? 0 : vbeg[big + 1] - vbeg[big];
    m->hull_large_set = large;
    m->hull_host.link.assign(link, link + nhulls);
    m->hull_host.vbeg.assign(vbeg, vbeg + nhulls + 1);
    m->hull_host.fbeg.assign(fbeg, fbeg + nhulls + 1);
    m->hull_host.pairs.assign(pairs, pairs + 2 * (size_t)npairs);
    m->hull_host.verts.assign(verts, verts + NV * 3);
    m->hull_host.planes.assign(planes, planes + NF * 4);
    m->hull_host.diam.assign(diam.begin(), diam.begin() + nhulls);
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
    if (m->hull_big < 0) return false;
    set_err(std::string(who) + ": hull " + std::to_string(m->hull_big) + " of the set has " + std::to_string(m->hull_big_nv) + " vertices, more than " +
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
    const auto &hh = m->hull_host;
    const int nhulls = m->hulls.nhulls, npairs = m->hulls.npairs;
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
    if (nmesh == 0) {
        m->hulls_plain = m->hulls;
        m->meshes = DevMeshes{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        m->meshg = DevMeshGrad{0, 0, nullptr, nullptr, nullptr};
        m->has_meshes = false;
        m->mesh_large = false;
        m->mesh_bvh = DevMeshBvh{nullptr, nullptr, nullptr};
        m->hulls_plain_big = m->hulls;
        return FBR_OK;
    }
    // the pairs of the set: those with a mesh on either side, the meshed hull first, sorted by it (stable); the others in their order
    std::vector<int> mtab((size_t)nhulls * 2, 0);
    for (int i = 0; i < nmesh; i++) mtab[2 * (size_t)hull[i]] = tbeg[i], mtab[2 * (size_t)hull[i] + 1] = tbeg[i + 1] - tbeg[i];
    // (a large attachment: the plain pairs of two hulls of at most FBR_MAX_HULL_VERTICES vertices in pk, the other plain pairs in bk --
    // the kernels they go to without meshes)
    std::vector<int> mk, pk, bk;
    const auto bighull = [&](int h) { return large && hh.vbeg[h + 1] - hh.vbeg[h] > FBR_MAX_HULL_VERTICES; };
    for (int k = 0; k < npairs; k++) {
        const int a = hh.pairs[2 * k], b = hh.pairs[2 * k + 1];
        (mtab[2 * (size_t)a + 1] || mtab[2 * (size_t)b + 1] ? mk : (bighull(a) || bighull(b) ? bk : pk)).push_back(k);
    }
    auto first = [&](int k) { return mtab[2 * (size_t)hh.pairs[2 * k] + 1] ? hh.pairs[2 * k] : hh.pairs[2 * k + 1]; };
    std::stable_sort(mk.begin(), mk.end(), [&](int a, int b) { return first(a) < first(b); });
    const size_t NT = (size_t)tbeg[nmesh], nm = std::max(mk.size(), (size_t)1), np = std::max(pk.size(), (size_t)1);
    // one allocation: sph | tris | aux | mesh pairs | plain pairs | mtab | mesh columns | plain columns
    FbrBlob blob;
    const size_t osph = blob.add<double>((size_t)nhulls * 4), otris = blob.add<double>(tris, tris + NT * 9), oaux = blob.add<double>(NT * 5);
    const size_t omp = blob.add<int>(2 * nm), opp = blob.add<int>(2 * np), omtab = blob.add<int>(mtab.begin(), mtab.end());
    const size_t omc = blob.add<int>(nm), opc = blob.add<int>(np);
    // (a large attachment: | big plain pairs | their columns | first node of a hull's tree | nodes | node spheres)
    const size_t nbp = std::max(bk.size(), (size_t)1);
    const size_t obp = blob.add<int>(2 * nbp), obc = blob.add<int>(nbp), onbeg = blob.add<int>((size_t)nhulls);
    const size_t onode = blob.add<int>(bvh.node.begin(), bvh.node.end()), ovol = blob.add<double>(bvh.vol.begin(), bvh.vol.end());
    for (size_t i = 0; i < bk.size(); i++)
        blob.at<int>(obp)[2 * i] = hh.pairs[2 * bk[i]], blob.at<int>(obp)[2 * i + 1] = hh.pairs[2 * bk[i] + 1], blob.at<int>(obc)[i] = bk[i];
    std::fill(blob.at<int>(onbeg), blob.at<int>(onbeg) + nhulls, 0);
    if (large)
        for (int i = 0; i < nmesh; i++) blob.at<int>(onbeg)[hull[i]] = bvh.nbeg[i];
    for (int h = 0; h < nhulls; h++)
        fbr_mesh_point_sphere(hh.vbeg[h + 1] - hh.vbeg[h], hh.verts.data() + 3 * (size_t)hh.vbeg[h], 3L * mtab[2 * (size_t)h + 1],
                              tris + 9 * (size_t)mtab[2 * (size_t)h], blob.at<double>(osph) + 4 * (size_t)h);
    for (size_t t = 0; t < NT; t++) fbr_mesh_triangle_aux(tris + 9 * t, blob.at<double>(oaux) + 5 * t);  // (large: what bvh.aux holds)
    int *hmp = blob.at<int>(omp), *hpp = blob.at<int>(opp), *hmc = blob.at<int>(omc), *hpc = blob.at<int>(opc);
    for (size_t i = 0; i < mk.size(); i++) {
        const int k = mk[i], a = hh.pairs[2 * k], b = hh.pairs[2 * k + 1], swap = mtab[2 * (size_t)a + 1] == 0;
        hmp[2 * i] = swap ? b : a, hmp[2 * i + 1] = swap ? a : b, hmc[i] = k;
    }
    for (size_t i = 0; i < pk.size(); i++) hpp[2 * i] = hh.pairs[2 * pk[i]], hpp[2 * i + 1] = hh.pairs[2 * pk[i] + 1], hpc[i] = pk[i];
    // the stencil points of fbr_mesh_distance_gradients (csrc/fbr_mesh_grad.h): per mesh pair the centre, then + eps, - eps of every joint
    // fbr_rigidgrad_item evaluates, in walk order: sbeg | pair of a point | its joint
    std::vector<int> gtab(mk.size() + 1, 0), gpair, gjoint;
    int smax = 0;
    if (!large) {  // (a large attachment has distances only)
        FbrKinIdProgram prog;
        if (int rc = collision_program(m, prog)) return rc;
        std::vector<int> stepof, anc, joint;
        fbr_capgrad_ancestors(m->hm, prog, stepof, anc);
        for (size_t i = 0; i < mk.size(); i++) {
            const int la = hh.link[hh.pairs[2 * mk[i]]], lb = hh.link[hh.pairs[2 * mk[i] + 1]];
            fbr_meshgrad_slots(la < 0 ? -1 : stepof[la], lb < 0 ? -1 : stepof[lb], m->hulls.fr.cmode, prog.steps.data(), anc.data(),
                               fbr_capgrad_words(prog.nsteps), joint);
            gtab[i + 1] = gtab[i] + (int)joint.size();
            gpair.insert(gpair.end(), joint.size(), (int)i);
            gjoint.insert(gjoint.end(), joint.begin(), joint.end());
            smax = std::max(smax, (int)joint.size());
        }
        gtab.insert(gtab.end(), gpair.begin(), gpair.end());
        gtab.insert(gtab.end(), gjoint.begin(), gjoint.end());
    } else {
        gtab.assign(1, 0);
    }
    // Unlike the three setters above, which reuse their buffers (they have cleared their set before they build), this one builds into fresh
    // allocations and swaps them in once the copies have succeeded: a call that fails here leaves the attachments in place as well.
    DevBuf fresh, freshg;
    if (int rc = upload_blob(fresh, blob)) return rc;
    if (int rc = freshg.ensure(gtab.size() * sizeof(int))) return rc;
    HIPCHK(hipMemcpy(freshg.p, gtab.data(), gtab.size() * sizeof(int), hipMemcpyHostToDevice));
    m->mesh_tab = std::move(fresh);
    m->meshg_tab = std::move(freshg);
    {
        const int *g = m->meshg_tab.as<int>();
        const int ni = (int)gpair.size();
        m->meshg = large ? DevMeshGrad{0, 0, nullptr, nullptr, nullptr} : DevMeshGrad{ni, smax, g, g + mk.size() + 1, g + mk.size() + 1 + ni};
    }
    m->hulls_plain = m->hulls;
    const char *base = (const char *)m->mesh_tab.p;
    m->meshes = DevMeshes{(int)mk.size(), (const int *)(base + omtab), (const double *)(base + osph), (const double *)(base + otris),
                          (const double *)(base + oaux), (const int2 *)(base + omp), (const int *)(base + omc)};
    m->hulls_plain.npairs = (int)pk.size();
    m->hulls_plain.pairs = (const int2 *)(base + opp);
    m->hulls_plain.col = (const int *)(base + opc);
    m->hulls_plain_big = m->hulls;
    m->hulls_plain_big.npairs = (int)bk.size();
    m->hulls_plain_big.pairs = (const int2 *)(base + obp);
    m->hulls_plain_big.col = (const int *)(base + obc);
    m->mesh_bvh = DevMeshBvh{(const int *)(base + onbeg), (const int *)(base + onode), (const double *)(base + ovol)};
    m->mesh_large = large;
    m->has_meshes = true;
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

// attachments of fbr_model_set_large_hull_meshes are in place: distances only, `who` has no gradients of them
static bool refuse_large_meshes(const fbr_model *m, const char *who)
{
    if (!(m->has_meshes && m->mesh_large)) return false;
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
    const bool have = m && m->hulls.nhulls != 0 && m->hulls.npairs != 0;
    const long P = m ? m->hulls.npairs : 0;
    return candidate_frame_distances(m, !m || have ? nullptr : "no hull set with at least one pair (fbr_model_set_hulls)", m ? m->hulls.fr : kNoBoxes, P,
                                     (P + FBR_HULL_BATCH - 1) / FBR_HULL_BATCH, st, base_pos, ncand, step, dist_out, idx_out, out_mem,
                                     [&](unsigned grid, const DevCapTiles &tl, long b0, long nb, const double *fr, double *pval, long *pidx) {
                                         const long cap = (long)m->num_cus * 32;
                                         const auto large = [&](const DevHulls &hs) {
                                             const long items = nb * ((hs.npairs + FBR_HULL_LARGE_BATCH - 1) / FBR_HULL_LARGE_BATCH);
                                             hipLaunchKernelGGL(fbr_hull_large_pairs_kernel, dim3((unsigned)std::min(items, cap)), dim3(64), 0, m->stream, hs, tl,
                                                                b0, nb, fr, pval, pidx);
                                         };
                                         if (m->has_meshes && m->mesh_large) {
                                             // attachments of fbr_model_set_large_hull_meshes: the pairs without a mesh to the kernels they go
                                             // to without any mesh, the others to the tree kernel, each into its own columns
                                             const long ps = m->hulls_plain.npairs, pb = m->hulls_plain_big.npairs, pm = m->meshes.npairs;
                                             const bool all = m->hull_large_set && m->opt.hull_large_all != 0;
                                             if (ps > 0 && all) large(m->hulls_plain);
                                             if (ps > 0 && !all)
                                                 hipLaunchKernelGGL(fbr_hull_pairs_kernel, dim3((unsigned)std::min(nb * ((ps + FBR_HULL_BATCH - 1) / FBR_HULL_BATCH), cap)),
                                                                    dim3(64), 0, m->stream, m->hulls_plain, tl, b0, nb, fr, pval, pidx);
                                             if (pb > 0) large(m->hulls_plain_big);
                                             if (pm > 0)
                                                 hipLaunchKernelGGL(fbr_mesh_bvh_pairs_kernel, dim3((unsigned)std::min(nb * pm, cap)), dim3(64), 0, m->stream,
                                                                    m->hulls, m->meshes, m->mesh_bvh, tl, b0, nb, fr, pval, pidx);
                                             return;
                                         }
                                         if (!m->has_meshes && m->hull_large_set && m->opt.hull_large_all != 0) {
                                             large(m->hulls);  // (every pair, in the caller's columns)
                                             return;
                                         }
                                         if (!m->has_meshes && m->hull_big >= 0) {
                                             // a set with large hulls: the pairs of two small hulls, then the others, each into its own columns
                                             const long ps = m->hulls_small.npairs;
                                             if (ps > 0)
                                                 hipLaunchKernelGGL(fbr_hull_pairs_kernel, dim3((unsigned)std::min(nb * ((ps + FBR_HULL_BATCH - 1) / FBR_HULL_BATCH), cap)),
                                                                    dim3(64), 0, m->stream, m->hulls_small, tl, b0, nb, fr, pval, pidx);
                                             if (m->hulls_big.npairs > 0) large(m->hulls_big);
                                             return;
                                         }
                                         if (!m->has_meshes) {
                                             hipLaunchKernelGGL(fbr_hull_pairs_kernel, dim3(grid), dim3(64), 0, m->stream, m->hulls, tl, b0, nb, fr, pval, pidx);
                                             return;
                                         }
                                         // a split set: the pairs without a mesh, then those with one, each into its own columns
                                         const long ph = m->hulls_plain.npairs, pm = m->meshes.npairs;
                                         if (ph > 0)
                                             hipLaunchKernelGGL(fbr_hull_pairs_kernel, dim3((unsigned)std::min(nb * ((ph + FBR_HULL_BATCH - 1) / FBR_HULL_BATCH), cap)),
                                                                dim3(64), 0, m->stream, m->hulls_plain, tl, b0, nb, fr, pval, pidx);
                                         if (pm > 0)
                                             hipLaunchKernelGGL(fbr_mesh_pairs_kernel, dim3((unsigned)std::min(nb * ((pm + FBR_MESH_BATCH - 1) / FBR_MESH_BATCH), cap)),
                                                                dim3(64), 0, m->stream, m->hulls, m->meshes, tl, b0, nb, fr, pval, pidx);
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
    if (m->hulls.nhulls == 0 || m->hulls.npairs == 0) {
        set_err("no hull set with at least one pair (fbr_model_set_hulls)");
        return FBR_E_INVALID;
    }
    if (refuse_large_meshes(m, "fbr_hull_distance_gradients")) return FBR_E_UNSUPPORTED;
    if (refuse_large_hulls(m, "fbr_hull_distance_gradients")) return FBR_E_INVALID;
    if (m->has_meshes) {
        set_err("fbr_hull_distance_gradients: the hull set has triangle meshes attached (fbr_model_set_hull_meshes); gradients of mesh pairs are not built");
        return FBR_E_UNSUPPORTED;
    }
    double se, omc;
    fbr_boxgrad_trig(epsilon, &se, &omc);
    return distance_gradients(m, "fbr_hull_distance_gradients", st, base_pos, ncand, sample, scale, pose_sample, dist_out, grad_q_out, out_mem,
                              m->hulls.npairs, m->hulls.fr.nslots,
                              [&](int grid, long C, long T, const double *dq, const double *drpy, const double *dbp, const long *dsmp, const double *dscale,
                                  const long *dpose, double *ddist, double *dgrad) {
                                  hipLaunchKernelGGL(fbr_hull_grad_kernel, dim3((unsigned)grid), dim3(64), 0, m->stream, m->dm, m->hulls, m->hullg, C, T, dq,
                                                     drpy, dbp, dsmp, dscale, dpose, epsilon, se, omc, ddist, dgrad, m->cap_scratch.as<double>(),
                                                     m->capg_flag.as<int>());
                                  return FBR_OK;
                              });
}

// A hull set with triangle meshes attached: the pairs without a mesh through fbr_hull_grad_kernel, into their columns; the pairs with one
// through the three stages of csrc/fbr_mesh_grad.h.
extern "C" int fbr_mesh_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                           const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out, double *grad_q_out,
                                           int32_t out_mem)
{
    if (!distance_gradient_args(m, st, sample, dist_out, grad_q_out, out_mem)) return FBR_E_INVALID;
    if (!std::isfinite(epsilon) || !(epsilon > 0.0)) {
        set_err("epsilon must be finite and positive");
        return FBR_E_INVALID;
    }
    if (m->hulls.nhulls == 0 || m->hulls.npairs == 0) {
        set_err("no hull set with at least one pair (fbr_model_set_hulls)");
        return FBR_E_INVALID;
    }
    if (refuse_large_meshes(m, "fbr_mesh_distance_gradients")) return FBR_E_UNSUPPORTED;
    if (refuse_large_hulls(m, "fbr_mesh_distance_gradients")) return FBR_E_INVALID;
    if (!m->has_meshes) {
        set_err("fbr_mesh_distance_gradients: the hull set has no triangle meshes attached (fbr_model_set_hull_meshes); fbr_hull_distance_gradients "
                "serves a set of hulls only");
        return FBR_E_INVALID;
    }
    double se, omc;
    fbr_boxgrad_trig(epsilon, &se, &omc);
    return distance_gradients(
        m, "fbr_mesh_distance_gradients", st, base_pos, ncand, sample, scale, pose_sample, dist_out, grad_q_out, out_mem, m->hulls.npairs, m->hulls.fr.nslots,
        [&](int grid, long C, long T, const double *dq, const double *drpy, const double *dbp, const long *dsmp, const double *dscale, const long *dpose,
            double *ddist, double *dgrad) -> int {
            const long tiles = (C + 63) / 64, ph = m->hulls_plain.npairs, pm = m->meshes.npairs, ni = m->meshg.nitems;
            if (ph > 0)
                hipLaunchKernelGGL(fbr_hull_grad_kernel, dim3((unsigned)std::min<long>(ph * tiles, grid)), dim3(64), 0, m->stream, m->dm, m->hulls_plain,
                                   m->hullg, C, T, dq, drpy, dbp, dsmp, dscale, dpose, epsilon, se, omc, ddist, dgrad, m->cap_scratch.as<double>(),
                                   m->capg_flag.as<int>());
            if (pm == 0) return FBR_OK;
            // the recorded poses [ni][13][C] | the stencil distances [ni][C]
            if (int rc = m->meshg_work.ensure((size_t)ni * (FBR_MESHGRAD_REL + 1) * (size_t)C * sizeof(double))) return rc;
            double *rel = m->meshg_work.as<double>(), *dv = rel + (size_t)ni * FBR_MESHGRAD_REL * (size_t)C;
            hipLaunchKernelGGL(fbr_mesh_grad_frames_kernel, dim3((unsigned)std::min<long>(pm * tiles, grid)), dim3(64), 0, m->stream, m->dm, m->hulls,
                               m->hullg, m->meshes, m->meshg, C, T, dq, drpy, dbp, dsmp, dscale, dpose, epsilon, se, omc, rel, m->cap_scratch.as<double>(),
                               m->capg_flag.as<int>());
            {
                ProfScope pb(m, FBR_PROF_REDUCE);  // (stage B by itself, inside the call's FBR_PROF_KIN)
                hipLaunchKernelGGL(fbr_mesh_grad_dist_kernel, dim3((unsigned)std::min<long>(ni * tiles, (long)m->num_cus * 32)), dim3(64), 0, m->stream,
                                   m->hulls, m->meshes, m->meshg, C, (const double *)rel, dv);
            }
            hipLaunchKernelGGL(fbr_mesh_grad_quot_kernel, dim3((unsigned)((C * pm + 255) / 256)), dim3(256), 0, m->stream, m->hulls, m->meshes, m->meshg,
                               (int)m->hm.n, C, T, dsmp, dpose, epsilon, (const double *)dv, ddist, dgrad);
            return FBR_OK;
        });
}

// A hull set installed by fbr_model_set_large_hulls: the pairs of two hulls of at most FBR_MAX_HULL_VERTICES vertices through
// fbr_hull_grad_kernel, into their columns; the large pairs -- every pair with option hull_large_all -- through the three stages of
// csrc/fbr_hull_large_grad.h.
extern "C" int fbr_large_hull_distance_gradients(fbr_model *m, const fbr_states *st, const double *base_pos, int32_t ncand, const int64_t *sample,
                                                 const double *scale, const int64_t *pose_sample, double epsilon, double *dist_out,
                                                 double *grad_q_out, int32_t out_mem)
{
    if (!distance_gradient_args(m, st, sample, dist_out, grad_q_out, out_mem)) return FBR_E_INVALID;
    if (!std::isfinite(epsilon) || !(epsilon > 0.0)) {
        set_err("fbr_large_hull_distance_gradients: epsilon must be finite and positive");
        return FBR_E_INVALID;
    }
    if (m->hulls.nhulls == 0 || !m->hull_large_set) {
        set_err("fbr_large_hull_distance_gradients: no hull set installed by fbr_model_set_large_hulls (fbr_hull_distance_gradients serves a set of "
                "fbr_model_set_hulls)");
        return FBR_E_INVALID;
    }
    if (m->hulls.npairs == 0) {
        set_err("fbr_large_hull_distance_gradients: the hull set has no pair");
        return FBR_E_INVALID;
    }
    if (refuse_large_meshes(m, "fbr_large_hull_distance_gradients")) return FBR_E_UNSUPPORTED;
    if (m->has_meshes) {  // (fbr_model_set_hull_meshes: only a set without a hull above the cap can have them)
        set_err("fbr_large_hull_distance_gradients: the hull set has triangle meshes attached (fbr_model_set_hull_meshes); "
                "fbr_mesh_distance_gradients serves such a set");
        return FBR_E_UNSUPPORTED;
    }
    const double wopt = m->opt.hull_grad_tile;
    if (!(wopt == 0 || wopt == 1 || wopt == 2 || wopt == 4 || wopt == 8 || wopt == 16 || wopt == 32 || wopt == 64)) {
        set_err("fbr_large_hull_distance_gradients: option hull_grad_tile must be 0 or a power of two from 1 to 64");
        return FBR_E_INVALID;
    }
    const bool all = m->opt.hull_large_all != 0;
    const int arr = all ? 1 : 0;
    const DevHulls none = DevHulls{kNoBoxes, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    const DevHulls hsmall = all ? none : (m->hull_big >= 0 ? m->hulls_small : m->hulls), hbig = all ? m->hulls : (m->hull_big >= 0 ? m->hulls_big : none);
    const DevMeshGrad lg = m->hull_lgrad[arr];
    const std::vector<int> &sbeg = m->hull_lgrad_sbeg[arr];
    double se, omc;
    fbr_boxgrad_trig(epsilon, &se, &omc);
    return distance_gradients(
        m, "fbr_large_hull_distance_gradients", st, base_pos, ncand, sample, scale, pose_sample, dist_out, grad_q_out, out_mem, m->hulls.npairs,
        m->hulls.fr.nslots,
        [&](int grid, long C, long T, const double *dq, const double *drpy, const double *dbp, const long *dsmp, const double *dscale, const long *dpose,
            double *ddist, double *dgrad) -> int {
            const long tiles = (C + 63) / 64, ps = hsmall.npairs, pl = hbig.npairs, ni = lg.nitems;
            if (ps > 0)
                hipLaunchKernelGGL(fbr_hull_grad_kernel, dim3((unsigned)std::min<long>(ps * tiles, grid)), dim3(64), 0, m->stream, m->dm, hsmall, m->hullg, C,
                                   T, dq, drpy, dbp, dsmp, dscale, dpose, epsilon, se, omc, ddist, dgrad, m->cap_scratch.as<double>(),
                                   m->capg_flag.as<int>());
            if (pl == 0) return FBR_OK;
            if ((long)sbeg.size() != pl + 1) {
                set_err("fbr_large_hull_distance_gradients: the stencil tables do not match the set");
                return FBR_E_INVALID;
            }
            // the recorded poses [ni][13][C] | the stencil distances [ni][C]
            if (int rc = m->hull_lgrad_work.ensure((size_t)ni * (FBR_MESHGRAD_REL + 1) * (size_t)C * sizeof(double))) return rc;
            double *rel = m->hull_lgrad_work.as<double>(), *dv = rel + (size_t)ni * FBR_MESHGRAD_REL * (size_t)C;
            hipLaunchKernelGGL(fbr_hull_large_grad_frames_kernel, dim3((unsigned)std::min<long>(pl * tiles, grid)), dim3(64), 0, m->stream, m->dm, hbig,
                               m->hullg, lg, C, T, dq, drpy, dbp, dsmp, dscale, dpose, epsilon, se, omc, rel, m->cap_scratch.as<double>(),
                               m->capg_flag.as<int>());
            const int width = wopt != 0 ? (int)wopt : fbr_hull_large_grad_width(sbeg.data(), (int)pl, C, (long)FBR_HULL_LARGE_GRAD_WAVES_PER_CU * m->num_cus);
            const long tpp = ((long)lg.smax * C + width - 1) / width;
            {
                ProfScope pb(m, FBR_PROF_REDUCE);  // (stage B by itself, inside the call's FBR_PROF_KIN)
                hipLaunchKernelGGL(fbr_hull_large_grad_dist_kernel, dim3((unsigned)std::min<long>(pl * tpp, (long)m->num_cus * 32)), dim3(64), 0, m->stream,
                                   hbig, lg, C, width, tpp, (const double *)rel, dv);
            }
            hipLaunchKernelGGL(fbr_hull_large_grad_quot_kernel, dim3((unsigned)((C * pl + 255) / 256)), dim3(256), 0, m->stream, hbig, lg, (int)m->hm.n, C, T,
                               dsmp, dpose, epsilon, (const double *)dv, ddist, dgrad);
            return FBR_OK;
        });
}
