// mesh_bvh_grad_sanitize.cpp -- a stand-alone program (TEST ONLY, built by tests/test_mesh_large_gradient.py with g++
// -fsanitize=address,undefined -fno-sanitize-recover=undefined and run on the CPU): the HIP-free text of csrc/fbr_mesh_bvh_grad.h and what
// fbr_large_mesh_distance_gradients builds on the host, on the case the test writes to its standard input.
//   1  the tables of a tree set: fbr_hull_pair_classes and the stencil tables of its MESH and BIG columns (fbr_stencil_table), their sizes
//      held against each other;
//   2  the entry mapping fbr_mesh_bvh_grad_entry / _entry_of in both orders at S of 1, 3, 63, 64 and 65 with C of 1 and 65: a bijection
//      onto [0, S) x [0, C); the tiles of fbr_mesh_bvh_grad_tile: every lane's entry inside the pair, every entry stored once;
//   3  the restatement (route 1) and the packets of both orders (routes 2, 3) of tests/emul/mesh_bvh_grad_emul.cpp against the single pass
//      (route 0), bit for bit.
// Prints "ok" and returns 0; the sanitizers abort on an out-of-bounds access, an overflow or a bad shift.
//
// Input, numbers separated by white space: L n, parent [L], dof [L], jtype [L], restR [9 L], restp [3 L], axis [3 L]; nhulls, link, offset
// [3 nhulls], rot [9 nhulls], vbeg [nhulls + 1], verts, fbeg, planes, ebeg, edges, mtab [2 nhulls], ntris, tris [9 ntris]; npairs, pairs
// [2 npairs] (the set's); C K, item pairs [2 C K], q [C K n].
#include <cstdio>
#include <iostream>

#include "mesh_bvh_grad_emul.cpp"
#include "../../flobaroid_amd/csrc/fbr_collision_tables.h"

template <class T> static std::vector<T> take(size_t n)
{
    std::vector<T> v(n);
    for (T &x : v) std::cin >> x;
    return v;
}

int main()
{
    int L = 0, n = 0, nhulls = 0;
    std::cin >> L >> n;
    const auto parent = take<int32_t>(L), dof = take<int32_t>(L), jtype = take<int32_t>(L);
    const auto restR = take<double>(9 * (size_t)L), restp = take<double>(3 * (size_t)L), axis = take<double>(3 * (size_t)L);
    std::cin >> nhulls;
    const auto link = take<int32_t>(nhulls);
    const auto offset = take<double>(3 * (size_t)nhulls), rot = take<double>(9 * (size_t)nhulls);
    const auto vbeg = take<int32_t>((size_t)nhulls + 1);
    const auto verts = take<double>(3 * (size_t)vbeg[nhulls]);
    const auto fbeg = take<int32_t>((size_t)nhulls + 1);
    const auto planes = take<double>(4 * (size_t)fbeg[nhulls]);
    const auto ebeg = take<int32_t>((size_t)nhulls + 1);
    const auto edges = take<int32_t>(4 * (size_t)ebeg[nhulls]);
    const auto mtab = take<int32_t>(2 * (size_t)nhulls);
    long ntris = 0;
    std::cin >> ntris;
    const auto tris = take<double>(9 * (size_t)ntris);
    int npairs = 0;
    std::cin >> npairs;
    const auto pairs = take<int32_t>(2 * (size_t)npairs);
    long C = 0, K = 0;
    std::cin >> C >> K;
    const auto item_pairs = take<int32_t>(2 * (size_t)(C * K));
    const auto q = take<double>((size_t)(C * K) * n);
    if (!std::cin) return printf("short input\n"), 1;

    // 1  the tables of a tree set
    FbrHostModel hm;
    const double g[3] = {0, 0, -9.81};
    hm.build(L, n, parent.data(), dof.data(), restR.data(), restp.data(), axis.data(), 0, g, 0, 1, 0, 0.0, nullptr, jtype.data());
    FbrKinIdProgram prog;
    fbr_kinid_build(hm, prog);
    std::vector<int> stepof, anc;
    fbr_capgrad_ancestors(hm, prog, stepof, anc);
    const std::vector<int> mt(mtab.begin(), mtab.end());
    const FbrPairClasses pc = fbr_hull_pair_classes(nhulls, vbeg.data(), mt.data(), npairs, pairs.data());
    if ((int)(pc.col[0].size() + pc.col[1].size() + pc.col[2].size()) != npairs) return printf("classes: %d pairs lost\n", npairs), 1;
    for (int cmode = 0; cmode < 2; cmode++)
        for (int cls : {FBR_PAIR_BIG, FBR_PAIR_MESH}) {
            const FbrStencilTable t = fbr_stencil_table(pc.col[cls], link.data(), stepof.data(), anc.data(), fbr_capgrad_words(prog.nsteps), cmode,
                                                        prog.steps.data(), pairs.data());
            if (t.npairs != (int)pc.col[cls].size() || (int)t.tab.size() != t.npairs + 1 + 2 * t.nitems || t.tab[t.npairs] != t.nitems)
                return printf("stencil table of class %d: sizes\n", cls), 1;
            for (int k = 0; k < t.npairs; k++) {
                const int s0 = t.tab[k], sk = t.tab[k + 1] - s0;
                if (sk < 1 || sk % 2 != 1 || sk > t.smax || t.tab[t.npairs + 1 + t.nitems + s0] != -1) return printf("stencil table: pair %d\n", k), 1;
                for (int s = 0; s < sk; s++)
                    if (t.tab[t.npairs + 1 + s0 + s] != k) return printf("stencil table: spair\n"), 1;
            }
        }

    // 2  the entry mapping
    long mapped = 0;
    for (int order : {FBR_MESH_GRAD_CANDIDATE_MAJOR, FBR_MESH_GRAD_SLOT_MAJOR})
        for (int S : {1, 3, 63, 64, 65})
            for (long Cc : {1L, 65L}) {
                const long E = (long)S * Cc;
                std::vector<char> seen((size_t)E, 0);
                for (long e = 0; e < E; e++) {
                    int s;
                    long c;
                    fbr_mesh_bvh_grad_entry(order, e, S, Cc, &s, &c);
                    if (s < 0 || s >= S || c < 0 || c >= Cc) return printf("entry %ld of %d x %ld, order %d: (%d, %ld) outside\n", e, S, Cc, order, s, c), 1;
                    if (fbr_mesh_bvh_grad_entry_of(order, s, c, S, Cc) != e) return printf("entry %ld: the inverse differs\n", e), 1;
                    if (seen[(size_t)s * Cc + c]++) return printf("entry %ld: (%d, %ld) twice\n", e, s, c), 1;
                    mapped++;
                }
                // the tiles of the pair as the kernel cuts them, tpp = ceil(E / 64) and one more: every lane's entry inside [0, E), every
                // entry stored by exactly one lane
                std::vector<char> stored((size_t)E, 0);
                const long tpp = (E + 63) / 64;
                for (long t = 0; t <= tpp; t++) {
                    long e0;
                    const int valid = fbr_mesh_bvh_grad_tile(t, E, &e0);
                    if ((t == tpp) != (valid == 0) || valid < 0 || valid > 64) return printf("tile %ld of %ld entries: %d\n", t, E, valid), 1;
                    for (int lane = 0; lane < 64 && valid; lane++) {
                        const long e = e0 + (lane < valid - 1 ? lane : valid - 1);
                        if (e < 0 || e >= E) return printf("tile %ld lane %d: entry %ld outside the pair's %ld\n", t, lane, e, E), 1;
                        if (lane < valid && stored[(size_t)e]++) return printf("entry %ld stored twice\n", e), 1;
                    }
                }
                for (long e = 0; e < E; e++)
                    if (!stored[(size_t)e]) return printf("entry %ld of %ld never stored\n", e, E), 1;
            }

    // 3  the four routes
    const long M = C * K;
    std::vector<double> dist[4], grad[4];
    std::vector<int32_t> ns((size_t)M);
    int64_t stats[6];
    for (int route = 0; route < 4; route++) {
        dist[route].assign((size_t)M, 0.0), grad[route].assign((size_t)M * n, 0.0);
        const int rc = meshbvhgrad_eval(L, n, parent.data(), dof.data(), restR.data(), restp.data(), axis.data(), jtype.data(), 0, nhulls, link.data(),
                                        offset.data(), rot.data(), 0, vbeg.data(), verts.data(), fbeg.data(), planes.data(), ebeg.data(), edges.data(),
                                        mtab.data(), tris.data(), ntris, 1e-7, C, K, item_pairs.data(), q.data(), nullptr, nullptr, route,
                                        dist[route].data(), grad[route].data(), ns.data(), stats, 0, nullptr);
        if (rc) return printf("route %d: %d\n", route, rc), 1;
        if (route > 0 && (std::memcmp(dist[route].data(), dist[0].data(), M * sizeof(double)) != 0 ||
                          std::memcmp(grad[route].data(), grad[0].data(), (size_t)M * n * sizeof(double)) != 0))
            return printf("route %d: not the bytes of the single pass\n", route), 1;
    }
    printf("ok %ld %ld\n", mapped, M);
    return 0;
}
