// gram64_rhs.cpp -- the rhs moments of the Gram pass over sample-contiguous images for k rhs columns (csrc/fbr_gram64.h: the producer's
// running sums fbr_gram64_mom_count / the reduction's index map fbr_gram64_mom_target), for tests/test_gram64_rhs.py (TEST ONLY).
// The host tables are built exactly as emul_gram64 of fbr_emul.cpp builds them, which this file includes; the producer is walked per
// (block, lane, part, link, parameter) like fbr_kinimg_kernel, the consumer is a plain contraction of the image over the tile pairs.
#include "fbr_emul.cpp"

extern "C" {
// G [(cols + k)^2], zeroed by the caller.  wstat: [0] / [1] fewest / most writers of a (column with a tile, rhs column) running sum per
// (block, live lane), [2] most writers of a sum of a column WITHOUT a tile, [3] columns with a tile, [4] fbr_gram64_mom_count.
// Returns -1 when the model is outside the pass, < -1 on an inconsistency of the tables.
int gram64_rhs(const EmulTopo *t, long S, const double *q, const double *dq, const double *ddq, const double *bv, const double *ba, const double *rpy,
               const double *sign, const double *rhs, int k, const double *wts, int force_tiles, double *G, long *wstat)
{
    FbrHostModel hm;
    make(t, hm);
    if (k < 1 || k > FBR_G64_MAXK || !fbr_gram_rhs_moments(hm, k)) return -1;
    FbrGramProgram gp;
    fbr_gram_build_best(gp, hm, k, g_shape, false);
    FbrGram64 g;
    FbrGram64Producer pr;
    if (!fbr_gram64_build(hm, gp, g, force_tiles != 0, false) || !fbr_gram64_build_producer(hm, g, pr)) return -1;
    const int P = hm.cols, Pa = P + k, NTT = g.NT + g.NF, nm = fbr_gram64_mom_count(P, k);
    std::vector<char> tiled(P, 0);
    for (int c : g.tilecol)
        if (c >= 0 && c < P) tiled[c] = 1;
    wstat[0] = 1 << 30;
    wstat[1] = wstat[2] = wstat[3] = 0;
    wstat[4] = nm;
    for (int c = 0; c < P; c++) wstat[3] += tiled[c];
    std::vector<double> rec(hm.rec_size()), img((size_t)g.blk_doubles), mom((size_t)nm * 64, 0.0);
    std::vector<int> writers(nm);
    const long nblk = (S + 63) / 64;
    for (long blk = 0; blk < nblk; blk++) {
        std::fill(img.begin(), img.end(), 0.0);
        const int valid = (int)std::min(64L, S - blk * 64);
        for (int lane = 0; lane < valid; lane++) {  // (the lanes behind the last sample take no part)
            const long s = blk * 64 + lane;
            kin_sample(hm, q + s * hm.n, dq + s * hm.n, ddq + s * hm.n, hm.floating ? bv + 6 * s : nullptr, hm.floating ? ba + 6 * s : nullptr,
                       hm.floating ? rpy + 3 * s : nullptr, rec.data());
            const double *ws = wts ? wts + (size_t)s * hm.rows : nullptr;
            auto wr = [&](int r) { return ws ? ws[r] : 1.0; };
            auto tv = [&](int r, int i) { return wr(r) * wr(r) * rhs[((size_t)s * hm.rows + r) * k + i]; };  // the staged w^2 rhs_i
            auto at = [&](long long dw, int lv) {
                return (long)((dw & ~(1LL << 62) & ~0xffLL) / 8) + (long)lv * 1024 + (lane >> 5) * 512 + ((lane & 31) ^ (int)(dw & 0xff));
            };
            std::fill(writers.begin(), writers.end(), 0);
            auto add = [&](int c, const double *mc) {  // one no-return atomic per (column, rhs column): this lane's own running sum
                for (int i = 0; i < k; i++) {
                    mom[(size_t)(i * P + c) * 64 + lane] += mc[i];
                    writers[i * P + c]++;
                }
            };
            for (int pq = 0; pq < pr.nparts; pq++)
                for (int l = 0; l < hm.L; l++) {
                    const long long *w14 = &pr.rel[((size_t)pq * hm.L + l) * FBR_G64_WORDS];
                    for (int pp = 0; pp < 10; pp++) {
                        const long long d0 = w14[pp], dF = pp < 4 ? w14[10 + pp] : 0;
                        if (!d0) continue;
                        const int c = pr.lcol[((size_t)pq * hm.L + l) * 10 + pp];
                        if (c < 0 || c >= P) return -2;
                        double w6[6], mc[FBR_G64_MAXK] = {0.0, 0.0};
                        fbr_unit_wrench(&rec[FBR_LINK_REC * l], pp, w6);
                        auto put = [&](long long dw, int lv, double v, int r) {
                            if (!dw || at(dw, lv) < 0 || at(dw, lv) >= g.blk_doubles) return false;
                            img[at(dw, lv)] = v * wr(r);
                            for (int i = 0; i < k; i++) mc[i] += v * tv(r, i);
                            return true;
                        };
                        for (int i = (pp >= 4 ? 3 : 0); i < hm.fb; i++)
                            if (!put(i < g.flev ? dF : d0, i, w6[i], i)) return -3;
                        int j = 0;
                        for (int d : hm.path[l]) {
                            if (!put(d0, hm.fb + j, fbr_dot6(&rec[FBR_LINK_REC * hm.L + 6 * d], w6), hm.fb + d)) return -3;
                            j++;
                        }
                        add(c, mc);
                    }
                    for (int pf = 0; pf < FBR_G64_FRIC; pf++) {
                        const long long dw = w14[14 + pf];
                        if (!dw) continue;
                        const int c = pr.lcol[(size_t)pr.nparts * 10 * hm.L + ((size_t)pq * hm.L + l) * FBR_G64_FRIC + pf];
                        if (c < hm.ninert || c >= P || hm.dof[l] != hm.coldesc[c].joint) return -4;
                        const int d = hm.dof[l], lv = hm.fb + (int)hm.path[l].size() - 1, r = hm.fb + d;
                        const double fv = fbr_friction_value(hm.coldesc[c].pidx, dq[s * hm.n + d], sign ? sign[s * hm.n + d] : 0.0, hm.stribeck);
                        if (at(dw, lv) < 0 || at(dw, lv) >= g.blk_doubles) return -3;
                        img[at(dw, lv)] = fv * wr(r);
                        double mc[FBR_G64_MAXK] = {0.0, 0.0};
                        for (int i = 0; i < k; i++) mc[i] = fv * tv(r, i);
                        add(c, mc);
                    }
                }
            // the corner (w rhs_i)^T (w rhs_j), i <= j, row by row: the last part's lane
            for (int i = 0, e = 0; i < k; i++)
                for (int j = i; j < k; j++, e++) {
                    double tt = 0.0;
                    for (int r = 0; r < hm.rows; r++)
                        tt += (rhs[((size_t)s * hm.rows + r) * k + i] * wr(r)) * (rhs[((size_t)s * hm.rows + r) * k + j] * wr(r));
                    mom[(size_t)(k * P + e) * 64 + lane] += tt;
                    writers[k * P + e]++;
                }
            for (int idx = 0; idx < nm; idx++) {
                const bool must = idx >= k * P || tiled[idx % P];
                if (must) {
                    wstat[0] = std::min<long>(wstat[0], writers[idx]);
                    wstat[1] = std::max<long>(wstat[1], writers[idx]);
                } else {
                    wstat[2] = std::max<long>(wstat[2], writers[idx]);
                }
            }
        }
        // consumer: every tile pair over its levels, all 64 sample slots of the block (the idle ones are zero)
        for (size_t sl = 0; sl + 2 < g.wmeta.size(); sl += 3) {
            const int tI = g.wmeta[sl], tJ = g.wmeta[sl + 1], lo = g.wmeta[sl + 2] & 0xff, hi = g.wmeta[sl + 2] >> 8;
            if (tI < 0) continue;
            for (int lv = lo; lv < hi; lv++) {
                const int trI = g.trow[(size_t)tI * g.nlev + lv], trJ = g.trow[(size_t)tJ * g.nlev + lv];
                if (trI < 0 || trJ < 0) return -6;
                for (int a = 0; a < FBR_TILE; a++)
                    for (int b = 0; b < FBR_TILE; b++) {
                        const int ci = g.tilecol[(size_t)tI * FBR_TILE + a], cj = g.tilecol[(size_t)tJ * FBR_TILE + b];
                        if (ci < 0 || cj < 0) continue;
                        double sum = 0.0;
                        for (int sm = 0; sm < 64; sm++)
                            sum += img[(size_t)trI * 1024 + (sm >> 5) * 512 + a * 32 + ((sm & 31) ^ FBR_G64_SWZ(a))] *
                                   img[(size_t)trJ * 1024 + (sm >> 5) * 512 + b * 32 + ((sm & 31) ^ FBR_G64_SWZ(b))];
                        G[(size_t)ci * Pa + cj] += sum;
                        if (tI != tJ) G[(size_t)cj * Pa + ci] += sum;
                    }
            }
        }
    }
    if (NTT <= 0) return -7;
    // fbr_gram64_mom_reduce_kernel: one sum per running sum, written where the index map says
    std::vector<char> hit((size_t)Pa * Pa, 0);
    for (int idx = 0; idx < nm; idx++) {
        double sum = 0.0;
        for (int lane = 0; lane < 64; lane++) sum += mom[(size_t)idx * 64 + lane];
        int row, col;
        fbr_gram64_mom_target(P, k, idx, &row, &col);
        if (row < 0 || col < P || col >= Pa || row > col || hit[(size_t)row * Pa + col]++) return -8;  // (every entry of the rhs block once)
        G[(size_t)row * Pa + col] += sum;
        if (row != col) G[(size_t)col * Pa + row] += sum;
    }
    for (int row = 0; row < Pa; row++)
        for (int col = std::max(row, P); col < Pa; col++)
            if (!hit[(size_t)row * Pa + col]) return -9;
    return 0;
}
}
