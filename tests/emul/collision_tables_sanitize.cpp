// collision_tables_sanitize.cpp -- a stand-alone program (TEST ONLY, built by tests/test_collision_tables.py with g++
// -fsanitize=address,undefined and run on the CPU): fbr_hull_pair_classes and fbr_stencil_table of csrc/fbr_collision_tables.h on the cases
// the test writes to its standard input, their results on the standard output for the test to hold against its restatement.  The sanitizers
// abort on an out-of-bounds access, an overflow or a bad shift.
//
// Input, numbers separated by white space: the tree -- L n, then parent [L], dof [L], jtype [L], restR [9 L], restp [3 L], axis [3 L] --,
// the count of cases, and per case: nhulls, link [nhulls], vbeg [nhulls + 1], 1 | 0 (a mesh table follows, or none), mtab [2 nhulls],
// npairs, pairs [2 npairs].
// Output per case: the counts of the three classes, then per class its columns, its pair list and (MESH) its swap flags; then for cmode 0
// and 1 and the column lists SMALL, BIG, MESH, every pair: npairs nitems smax and the table.  "ok" ends it.
#include <cstdio>
#include <iostream>
#include <numeric>
#include <vector>

#include "../../include/fbr.h"
#include "../../flobaroid_amd/csrc/fbr_collision_tables.h"

template <class T> static std::vector<T> take(size_t n)
{
    std::vector<T> v(n);
    for (T &x : v) std::cin >> x;
    return v;
}

static void put(const std::vector<int> &v)
{
    for (int x : v) printf(" %d", x);
    printf("\n");
}

int main()
{
    int L = 0, n = 0;
    std::cin >> L >> n;
    const auto parent = take<int32_t>(L), dof = take<int32_t>(L), jtype = take<int32_t>(L);
    const auto restR = take<double>(9 * (size_t)L), restp = take<double>(3 * (size_t)L), axis = take<double>(3 * (size_t)L);
    FbrHostModel hm;
    const double g[3] = {0, 0, -9.81};
    hm.build(L, n, parent.data(), dof.data(), restR.data(), restp.data(), axis.data(), 0, g, 0, 1, 0, 0.0, nullptr, jtype.data());
    FbrKinIdProgram prog;
    fbr_kinid_build(hm, prog);
    std::vector<int> stepof, anc;
    fbr_capgrad_ancestors(hm, prog, stepof, anc);
    int ncases = 0;
    std::cin >> ncases;
    for (int ic = 0; ic < ncases; ic++) {
        int nhulls = 0, has = 0, npairs = 0;
        std::cin >> nhulls;
        const auto link = take<int32_t>(nhulls), vbeg = take<int32_t>((size_t)nhulls + 1);
        std::cin >> has;
        const auto mtab = take<int>(has ? 2 * (size_t)nhulls : 0);
        std::cin >> npairs;
        const auto pairs = take<int32_t>(2 * (size_t)npairs);
        if (!std::cin) return printf("short input in case %d\n", ic), 1;
        const FbrPairClasses pc = fbr_hull_pair_classes(nhulls, vbeg.data(), has ? mtab.data() : nullptr, npairs, pairs.data());
        printf("%zu %zu %zu\n", pc.col[0].size(), pc.col[1].size(), pc.col[2].size());
        for (int c = 0; c < FBR_PAIR_CLASSES; c++) put(pc.col[c]), put(pc.pairs[c]);
        put(pc.swap);
        std::vector<int> every((size_t)npairs);
        std::iota(every.begin(), every.end(), 0);
        const std::vector<int> *cols[4] = {&pc.col[0], &pc.col[1], &pc.col[2], &every};
        for (int cmode = 0; cmode < 2; cmode++)
            for (int i = 0; i < 4; i++) {
                const FbrStencilTable t = fbr_stencil_table(*cols[i], link.data(), stepof.data(), anc.data(), fbr_capgrad_words(prog.nsteps), cmode,
                                                            prog.steps.data(), pairs.data());
                printf("%d %d %d\n", t.npairs, t.nitems, t.smax);
                put(t.tab);
            }
    }
    printf("ok\n");
    return 0;
}
