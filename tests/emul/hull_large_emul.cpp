// hull_large_emul.cpp -- the HIP-free text of csrc/fbr_hull_large.h on the CPU (TEST ONLY, built by tests/test_hulls_large.py with g++
// -ffp-contract=off): the distance as one lane of fbr_hull_large_pairs_kernel returns it -- GJK by the lane, the facet pass of a touching
// sample dealt into the wave's 64 parts, joined in lane order with the pass's own rule, kept by the sample's lane -- beside
// fbr_hull_distance, which walks the same facets in one loop, and the checks of fbr_model_set_large_hulls.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/fbr.h"
#include "../../flobaroid_amd/csrc/fbr_hull_large.h"

typedef FbrHullT<const double *, const int32_t *> Hull;

static Hull view(int h, const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges,
                 const double *diam)
{
    return Hull{vbeg[h + 1] - vbeg[h], fbeg[h + 1] - fbeg[h], ebeg[h + 1] - ebeg[h], verts + 3 * (size_t)vbeg[h], planes + 4 * (size_t)fbeg[h],
                edges + 4 * (size_t)ebeg[h], diam[h]};
}

extern "C" {

// dist [N], iters [N] (GJK iterations, + 1000: the facet pass ran) of N poses of ONE pair of hulls (tables of two hulls: 0 is A, 1 is B):
// R [N][9], c [N][3].  wave != 0: the facet pass as the wave shares it; 0: fbr_hull_distance.
void hull_large_distance(long N, const double *RA, const double *cA, const double *RB, const double *cB, const int32_t *vbeg, const double *verts,
                         const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges, const double *diam, int wave, double *dist,
                         int32_t *iters)
{
    const Hull A = view(0, vbeg, verts, fbeg, planes, ebeg, edges, diam), B = view(1, vbeg, verts, fbeg, planes, ebeg, edges, diam);
    for (long i = 0; i < N; i++) {
        int it = 0;
        dist[i] = wave ? fbr_hull_large_distance(RA + 9 * i, cA + 3 * i, A, RB + 9 * i, cB + 3 * i, B, &it)
                       : fbr_hull_distance(RA + 9 * i, cA + 3 * i, A, RB + 9 * i, cB + 3 * i, B, &it);
        iters[i] = it;
    }
}

// the 64 partial maxima part [N][64] of the facet pass of N poses (whether they touch or not): what the lanes hold before they are joined
void hull_large_parts(long N, const double *RA, const double *cA, const double *RB, const double *cB, const int32_t *vbeg, const double *verts,
                      const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges, const double *diam, double *part)
{
    const Hull A = view(0, vbeg, verts, fbeg, planes, ebeg, edges, diam), B = view(1, vbeg, verts, fbeg, planes, ebeg, edges, diam);
    for (long i = 0; i < N; i++) {
        FbrHullRel q;
        fbr_hull_relative(RA + 9 * i, cA + 3 * i, RB + 9 * i, cB + 3 * i, &q);
        for (int l = 0; l < FBR_HULL_LARGE_PARTS; l++) part[i * FBR_HULL_LARGE_PARTS + l] = fbr_hull_facets(q, A, B, l, FBR_HULL_LARGE_PARTS);
    }
}

// 0 when fbr_model_set_large_hulls (large != 0) or fbr_model_set_hulls (0) would accept the set on a model of L links, else -1 and the message
int hull_large_validate(int L, int large, int nhulls, const int32_t *link, const double *offset, const double *rot, const int32_t *vbeg, const double *verts,
                        const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges, int npairs, const int32_t *pairs, char *msg,
                        int len)
{
    const std::string e = fbr_hull_validate(L, FBR_MAX_HULLS, FBR_MAX_HULL_PAIRS, large ? FBR_MAX_LARGE_HULL_VERTICES : FBR_MAX_HULL_VERTICES, nhulls, link,
                                            offset, rot, vbeg, verts, fbeg, planes, ebeg, edges, npairs, pairs, nullptr);
    if (msg && len > 0) {
        strncpy(msg, e.c_str(), len - 1);
        msg[len - 1] = 0;
    }
    return e.empty() ? 0 : -1;
}

int hull_large_key_bits(void) { return FBR_HULL_KEY_BITS; }
}
