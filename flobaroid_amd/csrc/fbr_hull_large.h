// fbr_hull_large.h -- convex hulls of 129 to FBR_MAX_LARGE_HULL_VERTICES vertices (fbr_model_set_large_hulls): the pairs kernel of
// fbr_candidate_hull_distances for pairs with such a hull.  KUKA LWR4 has visual meshes only, whose hulls have 158 to 793 vertices, 196 to
// 1481 faces and 352 to 2272 edges ("Large convex hulls").
//
// The distance is fbr_hull_distance's (csrc/fbr_hull.h), evaluated in two parts:
//   * GJK, one lane per sample as in fbr_hull_pairs_kernel: the support scans have wave-uniform counters and scalar loads, V_A + V_B steps
//     an iteration, and end after FBR_HULL_MAX_ITER iterations at the latest;
//   * the facet pass of a touching sample, E_A E_B arc tests (4.1e6 for link_4 against link_6), which one lane cannot carry while 63 wait:
//     the wave takes the touching samples one after the other, in ascending lane order.  The sample's relative pose is broadcast exactly
//     (v_readlane on the 13 doubles), lane l calls fbr_hull_facets(q, A, B, l, 64) -- the faces of A, the faces of B and the edges of B with
//     index l modulo 64, each edge of B against every edge of A --, and the 64 partial maxima are joined in lane order with the rule of the
//     pass itself (g > gap: a NaN is never taken).  The sample's lane keeps the result.  No atomics: every run returns the same bits, and
//     fbr_hull_facets_wave below is the same sequence on the host (tests/emul/hull_large_emul.cpp).  A maximum does not depend on how the
//     facets are dealt out, so the value equals fbr_hull_distance's; the sign of a zero gap is the only thing the order can change.
#pragma once
#include "fbr_hull.h"

#define FBR_HULL_LARGE_PARTS 64  // the parts the facet pass of one sample is dealt into: the lanes of a wave

// the wave's facet pass as the host walks it: part 0, 1, .. 63 joined in that order
template <class DP, class IP>
inline double fbr_hull_facets_wave(const FbrHullRel &q, const FbrHullT<DP, IP> &A, const FbrHullT<DP, IP> &B)
{
    double gap = -1e300;
    for (int l = 0; l < FBR_HULL_LARGE_PARTS; l++) {
        const double g = fbr_hull_facets(q, A, B, l, FBR_HULL_LARGE_PARTS);
        gap = g > gap ? g : gap;
    }
    return gap;
}

// fbr_hull_distance with the facet pass dealt into the wave's parts (the host's restatement of one lane of fbr_hull_large_pairs_kernel)
template <class DP, class IP>
inline double fbr_hull_large_distance(const double *RA, const double *cA, const FbrHullT<DP, IP> &A, const double *RB, const double *cB,
                                      const FbrHullT<DP, IP> &B, int *iters)
{
    FbrHullRel q;
    fbr_hull_relative(RA, cA, RB, cB, &q);
    bool touching;
    int it;
    const double res = fbr_hull_gjk(q, A, B, false, &touching, &it);
    if (iters) *iters = it + (touching ? 1000 : 0);
    return touching ? fbr_hull_facets_wave(q, A, B) : res;
}

#if defined(__HIPCC__)
#define FBR_HULL_LARGE_BATCH 4  // pairs a wave stages in the LDS: a large pair is 10 to 1e4 small pairs' work, small batches spread it over the CUs

#if defined(FBR_KERNELS_COLLISION)
// x of lane s (wave-uniform), bit for bit
__device__ __forceinline__ double fbr_lane_value(double x, int s)
{
    const long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffL), s), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), s);
    return __longlong_as_double((long)(((unsigned long)hi << 32) | lo));
}

// The facet pass of the touching lanes `todo` (wave-uniform) of a wave whose lanes hold the poses q of one pair of hulls, one lane after
// the other in ascending order: the pose of lane s broadcast exactly, lane l on fbr_hull_facets(q_s, A, B, l, 64), the 64 partial maxima
// joined in lane order with g > gap.  Returns d, in a touching lane the gap of its pose.
__device__ __forceinline__ double fbr_hull_large_touching(unsigned long todo, const FbrHullRel &q, const FbrDevHull &HA, const FbrDevHull &HB, int lane,
                                                          double d)
{
#pragma unroll 1
    while (todo != 0) {
        const int s = (int)__builtin_ctzl(todo);
        todo &= todo - 1;
        FbrHullRel qs;
        qs.t0 = fbr_lane_value(q.t0, s), qs.t1 = fbr_lane_value(q.t1, s), qs.t2 = fbr_lane_value(q.t2, s);
        qs.C00 = fbr_lane_value(q.C00, s), qs.C01 = fbr_lane_value(q.C01, s), qs.C02 = fbr_lane_value(q.C02, s);
        qs.C10 = fbr_lane_value(q.C10, s), qs.C11 = fbr_lane_value(q.C11, s), qs.C12 = fbr_lane_value(q.C12, s);
        qs.C20 = fbr_lane_value(q.C20, s), qs.C21 = fbr_lane_value(q.C21, s), qs.C22 = fbr_lane_value(q.C22, s);
        qs.chk = fbr_lane_value(q.chk, s);
        const double g = fbr_hull_facets(qs, HA, HB, lane, FBR_HULL_LARGE_PARTS);
        double gap = -1e300;
#pragma unroll
        for (int l = 0; l < FBR_HULL_LARGE_PARTS; l++) {
            const double x = fbr_lane_value(g, l);
            gap = x > gap ? x : gap;
        }
        if (lane == s) d = gap;
    }
    return d;
}

// work items (block, batch of FBR_HULL_LARGE_BATCH pairs), one wave each, one lane per checked sample; pval / pidx [nb][hs.ldp], the
// pair's column hs.col[pair] (null: its own number), as for fbr_hull_pairs_kernel.  Every loop is bounded by the hull tables, the 64 bits
// of the ballot and FBR_HULL_MAX_ITER.
__global__ __launch_bounds__(64) void fbr_hull_large_pairs_kernel(DevHulls hs, DevCapTiles tl, long blk0, long nb, const double *__restrict__ fr,
                                                                  double *__restrict__ pval, long *__restrict__ pidx)
{
    __shared__ double sd[FBR_HULL_LARGE_BATCH * 65];
    const int lane = threadIdx.x;
    const long nbatch = (hs.npairs + FBR_HULL_LARGE_BATCH - 1) / FBR_HULL_LARGE_BATCH, items = nb * nbatch;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const FbrPairItem w = fbr_pair_item(it, nbatch, FBR_HULL_LARGE_BATCH, hs.npairs, tl, blk0);
        // lanes behind the last checked sample repeat it, as in fbr_hull_pairs_kernel: they walk its GJK and are never scanned
        const double *f = fr + w.b * (long)hs.fr.nrob * 12 * 64 + min(lane, w.valid - 1);
        int cura = 0;
        bool have = false;
        double RA[9], cA[3];
        FbrDevHull HA = {0, 0, 0, nullptr, nullptr, nullptr, 0.0};
        for (int i = 0; i < 9; i++) RA[i] = 0.0;
        for (int i = 0; i < 3; i++) cA[i] = 0.0;
        __syncthreads();  // (the item before has been scanned)
#pragma unroll 1
        for (int j = 0; j < w.cnt; j++) {
            const fbr_cint_ptr pr = (fbr_cint_ptr)(unsigned long)(hs.pairs + w.k0 + j);
            const int ia = FBR_UNI(pr[0]), ib = FBR_UNI(pr[1]);
            if (!have || ia != cura) {
                fbr_hull_fetch(hs, ia, f, RA, cA, &HA);
                cura = ia;
                have = true;
            }
            double RB[9], cB[3];
            FbrDevHull HB;
            fbr_hull_fetch(hs, ib, f, RB, cB, &HB);
            FbrHullRel q;
            fbr_hull_relative(RA, cA, RB, cB, &q);
            bool touching;
            int iters;
            double d = fbr_hull_gjk(q, HA, HB, false, &touching, &iters);
            // the touching samples, one after the other (the repeats behind the last checked sample are not counted)
            const unsigned long todo = __builtin_amdgcn_ballot_w64(touching && lane < w.valid);
            d = fbr_hull_large_touching(todo, q, HA, HB, lane, d);
            sd[j * 65 + lane] = d;
        }
        __syncthreads();
        fbr_pair_scan_store(sd, w, lane, tl, hs.ldp, [&](int k) { return hs.col ? hs.col[k] : k; }, pval, pidx);
    }
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
