// fbr_collision_tables.h -- the host tables every collision set shares (fbr_model_set_capsules, fbr_model_set_boxes, fbr_model_set_hulls in
// fbr_collision_api.hip): the members sorted by the step of their link, the per-pair table of the gradient calls, and the one allocation a
// set's arrays are packed into.  HIP-free: tests/test_collision_tables.py compiles it with g++ and holds it against a restatement.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "fbr_capsule_grad.h"

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
