// collision_tables_emul.cpp -- csrc/fbr_collision_tables.h on the CPU (TEST ONLY, built by tests/test_collision_tables.py with g++): the
// step sort, the slot numbers and the gradient table of a collision set, on the step program the library builds (fbr_kinid_build); the
// classes of a hull set's pairs and the stencil tables of its staged gradient calls.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/fbr.h"
#include "../../flobaroid_amd/csrc/fbr_collision_tables.h"

extern "C" {

// link [nmem] (-1: a world member), pairs [npairs][2] member numbers.  Out: steplink [L] the link of every step (returns their count),
// stepof [L], beg [L + 1], code / slot [nmem], id [max(nrob, 1)], counts = {nrob, nworld, W}, gt [4 max(npairs, 1) + nsteps W].
int collision_tables(int L, int n, const int32_t *parent, const int32_t *dof, const double *restR, const double *restp, const double *axis,
                     const int32_t *jtype, int nmem, const int32_t *link, int npairs, const int32_t *pairs, int32_t *steplink, int32_t *stepof,
                     int32_t *beg, int32_t *code, int32_t *slot, int32_t *id, int32_t *counts, int32_t *gt)
{
    FbrHostModel hm;
    const double g[3] = {0, 0, -9.81};
    try {
        hm.build(L, n, parent, dof, restR, restp, axis, 0, g, 0, 1, 0, 0.0, nullptr, jtype);
    } catch (...) {
        return -1;
    }
    FbrKinIdProgram prog;
    fbr_kinid_build(hm, prog);
    FbrCollisionSort s;
    fbr_collision_sort(hm, prog, nmem, link, s);
    const std::vector<int> t = fbr_collision_grad_table(s, link, npairs, pairs);
    if ((int)s.beg.size() != prog.nsteps + 1 || (int)s.id.size() != std::max(s.nrob, 1) || (int)s.stepof.size() != L) return -2;
    if (t.size() != (size_t)4 * std::max(npairs, 1) + (size_t)prog.nsteps * s.W) return -3;
    for (int k = 0; k < prog.nsteps; k++) steplink[k] = prog.steps[(size_t)k * FBR_KINID_STEP];
    std::copy(s.stepof.begin(), s.stepof.end(), stepof);
    std::copy(s.beg.begin(), s.beg.end(), beg);
    std::copy(s.code.begin(), s.code.end(), code);
    std::copy(s.slot.begin(), s.slot.end(), slot);
    std::copy(s.id.begin(), s.id.end(), id);
    counts[0] = s.nrob, counts[1] = s.nworld, counts[2] = s.W;
    std::copy(t.begin(), t.end(), gt);
    return prog.nsteps;
}

// nd doubles, ni ints, np int2 pairs packed as the setters pack them: off = offsets of the three arrays, returns the size; the doubles
// count up from 1, the ints from 100, the pairs from 1000 (out: the bytes, at least 8 (nd + ni + 2 np + 1) of them).
long collision_blob(int nd, int ni, int np, long *off, char *out)
{
    std::vector<double> d(nd);
    std::vector<int> iv(ni), pv(2 * (size_t)np);
    for (int i = 0; i < nd; i++) d[i] = 1 + i;
    for (int i = 0; i < ni; i++) iv[i] = 100 + i;
    FbrBlob b;
    off[0] = (long)b.add<double>(d.begin(), d.end());
    off[1] = (long)b.add<int>(iv.begin(), iv.end());
    off[2] = (long)b.add<int>(pv.size(), 8);
    for (size_t i = 0; i < pv.size(); i++) b.at<int>(off[2])[i] = 1000 + (int)i;
    std::copy(b.bytes.begin(), b.bytes.end(), out);
    return (long)b.bytes.size();
}
// fbr_hull_pair_classes: vbeg [nhulls + 1], mtab [nhulls][2] or null, pairs [npairs][2].  Out, a class after the other (SMALL, BIG, MESH):
// counts [3], col [npairs], list [npairs][2], swap [npairs] by the place in col (-1 outside MESH).
void hull_pair_classes(int nhulls, const int32_t *vbeg, const int32_t *mtab, int npairs, const int32_t *pairs, int32_t *counts, int32_t *col,
                       int32_t *list, int32_t *swap)
{
    const FbrPairClasses pc = fbr_hull_pair_classes(nhulls, vbeg, mtab, npairs, pairs);
    size_t o = 0;
    for (int c = 0; c < FBR_PAIR_CLASSES; c++) {
        counts[c] = (int)pc.col[c].size();
        for (size_t i = 0; i < pc.col[c].size(); i++, o++) {
            col[o] = pc.col[c][i];
            list[2 * o] = pc.pairs[c].at(2 * i), list[2 * o + 1] = pc.pairs[c].at(2 * i + 1);
            swap[o] = c == FBR_PAIR_MESH ? pc.swap.at(i) : -1;
        }
    }
}

// fbr_stencil_table of ncols columns of a set of hulls on `link` (-1: a world hull), on the program of the tree given as for
// collision_tables.  Out: tab [cap] = sbeg | spair | sjoint, counts = {npairs, nitems, smax}, direct [ncols] = the size of
// fbr_meshgrad_slots of every column's pair by itself.  Returns the entries of tab, -1: the tree, -2: cap is too small.
int stencil_table(int L, int n, const int32_t *parent, const int32_t *dof, const double *restR, const double *restp, const double *axis,
                  const int32_t *jtype, const int32_t *link, const int32_t *pairs, int ncols, const int32_t *cols, int cmode, int cap, int32_t *tab,
                  int32_t *counts, int32_t *direct)
{
    FbrHostModel hm;
    const double g[3] = {0, 0, -9.81};
    try {
        hm.build(L, n, parent, dof, restR, restp, axis, 0, g, 0, 1, 0, 0.0, nullptr, jtype);
    } catch (...) {
        return -1;
    }
    FbrKinIdProgram prog;
    fbr_kinid_build(hm, prog);
    std::vector<int> stepof, anc, joint;
    fbr_capgrad_ancestors(hm, prog, stepof, anc);
    const int W = fbr_capgrad_words(prog.nsteps);
    const FbrStencilTable t = fbr_stencil_table(std::vector<int>(cols, cols + ncols), link, stepof.data(), anc.data(), W, cmode, prog.steps.data(), pairs);
    if ((int)t.tab.size() > cap) return -2;
    std::copy(t.tab.begin(), t.tab.end(), tab);
    counts[0] = t.npairs, counts[1] = t.nitems, counts[2] = t.smax;
    for (int i = 0; i < ncols; i++) {
        const int la = link[pairs[2 * cols[i]]], lb = link[pairs[2 * cols[i] + 1]];
        fbr_meshgrad_slots(la < 0 ? -1 : stepof[la], lb < 0 ? -1 : stepof[lb], cmode, prog.steps.data(), anc.data(), W, joint);
        direct[i] = (int)joint.size();
    }
    return (int)t.tab.size();
}
}
