// fbr_collision_tables.h -- the host tables every collision set shares (fbr_model_set_capsules, fbr_model_set_boxes, fbr_model_set_hulls in
// fbr_collision_api.hip): the members sorted by the step of their link, the per-pair table of the gradient calls, and the one allocation a
// set's arrays are packed into; for the hull set the classes of its pairs and the stencil tables of the staged gradient calls.  HIP-free:
// tests/test_collision_tables.py compiles it with g++ and holds it against a restatement.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/fbr.h"  // FBR_MAX_HULL_VERTICES
#include "fbr_capsule_grad.h"
#include "fbr_mesh_grad.h"

// Members of a set (capsules, boxes, hulls) by the link they sit on; link < 0: a world member.
struct FbrCollisionSort {
    int nrob = 0, nworld = 0;
    int W = 0;                // words per row of anc (fbr_capgrad_words)
    std::vector<int> stepof;  // [L] step of a link in the program
    std::vector<int> anc;     // [nsteps][W] (fbr_capgrad_ancestors)
    std::vector<int> code;    // [members] robot-member number (the caller's order among the members with a link), or -1 - (world-member number)
    std::vector<int> beg;     // [nsteps + 1] slots of every step: the robot members sorted by the step of their link, stable
    std::vector<int> slot;    // [members] slot of a robot member (a world member: -1)
    std::vector<int> id;      // [max(nrob, 1)] slot -> robot-member number
};

static inline void fbr_collision_sort(const FbrHostModel &hm, const FbrKinIdProgram &prog, int nmem, const int32_t *link, FbrCollisionSort &s)
{
    s.nrob = s.nworld = 0;
    s.W = fbr_capgrad_words(prog.nsteps);
    fbr_capgrad_ancestors(hm, prog, s.stepof, s.anc);
    s.code.resize(nmem);
    s.beg.assign(prog.nsteps + 1, 0);
    for (int c = 0; c < nmem; c++) {
        s.code[c] = link[c] < 0 ? -1 - s.nworld++ : s.nrob++;
        if (link[c] >= 0) s.beg[s.stepof[link[c]] + 1]++;
    }
    for (int k = 0; k < prog.nsteps; k++) s.beg[k + 1] += s.beg[k];
    std::vector<int> fill(s.beg.begin(), s.beg.end() - 1);
    s.slot.assign(nmem, -1);
    s.id.assign(std::max(s.nrob, 1), 0);
    for (int c = 0; c < nmem; c++)
        if (link[c] >= 0) {
            s.slot[c] = fill[s.stepof[link[c]]]++;
            s.id[s.slot[c]] = s.code[c];
        }
}

// The table of the gradient calls: per pair (the caller's member numbers) step_a, step_b, slot_a, slot_b -- a world member: -1 and its
// world number -- for max(npairs, 1) pairs, followed by the ancestor masks.
static inline std::vector<int> fbr_collision_grad_table(const FbrCollisionSort &s, const int32_t *link, int npairs, const int32_t *pairs)
{
    const size_t np = (size_t)std::max(npairs, 1);
    std::vector<int> gt(4 * np + s.anc.size(), 0);
    for (int k = 0; k < npairs; k++)
        for (int j = 0; j < 2; j++) {
            const int c = pairs[2 * k + j];
            gt[4 * (size_t)k + j] = link[c] < 0 ? -1 : s.stepof[link[c]];
            gt[4 * (size_t)k + 2 + j] = link[c] < 0 ? -1 - s.code[c] : s.slot[c];
        }
    std::copy(s.anc.begin(), s.anc.end(), gt.begin() + 4 * np);
    return gt;
}

// ---- the hull set: which pair goes to which kernel ("Hull set: classes, views, stencils") ---------------------------------------
// The class of a pair, decided in this order: MESH if either hull carries triangles, else BIG if either hull has more than
// FBR_MAX_HULL_VERTICES vertices (include/fbr.h), else SMALL.
enum { FBR_PAIR_SMALL = 0, FBR_PAIR_BIG = 1, FBR_PAIR_MESH = 2, FBR_PAIR_CLASSES = 3 };

struct FbrPairClasses {
    std::vector<int> col[FBR_PAIR_CLASSES];    // the caller's column of every pair of the class, in the caller's order -- MESH: in the list's
    std::vector<int> pairs[FBR_PAIR_CLASSES];  // [2 x] the hull numbers the kernels read.  MESH: the meshed hull first (both meshed: the caller's
                                               // order), sorted by it, stable
    std::vector<int> swap;                     // per MESH pair: 1 when the list has the caller's members exchanged (the mesh is the second's)
};

// vbeg [nhulls + 1]; mtab [nhulls][2] first triangle | count (0: no mesh) or null: no meshes; pairs [npairs][2] the caller's hull numbers
static inline FbrPairClasses fbr_hull_pair_classes(int /*nhulls*/, const int32_t *vbeg, const int *mtab, int npairs, const int32_t *pairs)
{
    const auto meshed = [&](int h) { return mtab && mtab[2 * (size_t)h + 1] != 0; };
    const auto big = [&](int h) { return vbeg[h + 1] - vbeg[h] > FBR_MAX_HULL_VERTICES; };
    FbrPairClasses pc;
    for (int k = 0; k < npairs; k++) {
        const int a = pairs[2 * k], b = pairs[2 * k + 1];
        pc.col[meshed(a) || meshed(b) ? FBR_PAIR_MESH : (big(a) || big(b) ? FBR_PAIR_BIG : FBR_PAIR_SMALL)].push_back(k);
    }
    std::vector<int> &mk = pc.col[FBR_PAIR_MESH];
    const auto first = [&](int k) { return meshed(pairs[2 * k]) ? pairs[2 * k] : pairs[2 * k + 1]; };
    std::stable_sort(mk.begin(), mk.end(), [&](int a, int b) { return first(a) < first(b); });
    for (int c = 0; c < FBR_PAIR_CLASSES; c++)
        for (int k : pc.col[c]) {
            const bool sw = c == FBR_PAIR_MESH && !meshed(pairs[2 * k]);
            pc.pairs[c].push_back(pairs[2 * k + (sw ? 1 : 0)]);
            pc.pairs[c].push_back(pairs[2 * k + (sw ? 0 : 1)]);
            if (c == FBR_PAIR_MESH) pc.swap.push_back(sw ? 1 : 0);
        }
    return pc;
}

// The stencil points of the staged gradient calls (csrc/fbr_mesh_grad.h, fbr_hull_large_grad.h) for a list of columns: per pair the centre,
// then + eps, - eps of every joint fbr_rigidgrad_item evaluates, in walk order (fbr_meshgrad_slots on the pair's own, unswapped members).
// tab: sbeg [columns + 1] | spair [nitems] the place of a point's pair in the list | sjoint [nitems] the joint it moves (-1: the centre).
struct FbrStencilTable {
    int npairs = 0, nitems = 0, smax = 0;
    std::vector<int> tab;
};

// link [nhulls] (-1: a world hull); stepof, anc, W: fbr_capgrad_ancestors; cmode: the set's offset_in_link_axes; steps: the step program;
// pairs: the caller's
static inline FbrStencilTable fbr_stencil_table(const std::vector<int> &columns, const int32_t *link, const int *stepof, const int *anc, int W, int cmode,
                                                const int *steps, const int32_t *pairs)
{
    FbrStencilTable t;
    t.npairs = (int)columns.size();
    t.tab.assign(1, 0);
    std::vector<int> spair, sjoint, joint;
    for (size_t i = 0; i < columns.size(); i++) {
        const int la = link[pairs[2 * columns[i]]], lb = link[pairs[2 * columns[i] + 1]];
        fbr_meshgrad_slots(la < 0 ? -1 : stepof[la], lb < 0 ? -1 : stepof[lb], cmode, steps, anc, W, joint);
        t.tab.push_back(t.tab.back() + (int)joint.size());
        spair.insert(spair.end(), joint.size(), (int)i);
        sjoint.insert(sjoint.end(), joint.begin(), joint.end());
        t.smax = std::max(t.smax, (int)joint.size());
    }
    t.nitems = (int)spair.size();
    t.tab.insert(t.tab.end(), spair.begin(), spair.end());
    t.tab.insert(t.tab.end(), sjoint.begin(), sjoint.end());
    return t;
}

// One allocation of several arrays: add() reserves n zeroed elements at the element's alignment (or a wider one: the int2 pairs behind the
// ints) and returns their offset; the doubles go first, so that every table keeps its alignment.
struct FbrBlob {
    std::vector<char> bytes;
    template <class T> size_t add(size_t n, size_t align = sizeof(T))
    {
        const size_t off = (bytes.size() + align - 1) / align * align;
        bytes.resize(off + n * sizeof(T), 0);
        return off;
    }
    template <class T, class It> size_t add(It first, It last, size_t align = sizeof(T))
    {
        const size_t off = add<T>((size_t)(last - first), align);
        std::copy(first, last, (T *)(bytes.data() + off));
        return off;
    }
    template <class T> T *at(size_t off) { return (T *)(bytes.data() + off); }
};
