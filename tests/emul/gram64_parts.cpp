// gram64_parts.cpp -- the producer's parts of the sample-contiguous Gram pass (csrc/fbr_gram64.h fbr_gram64_build_producer: options
// gram_lane_skip_unowned, gram_lane_parts_cut) and its chunk sizes (fbr_gram64_chunk_plan, option gram_lane_chunk_rounds), for
// tests/test_gram64_parts.py (TEST ONLY).  It builds the program exactly as emul_gram64 of fbr_emul.cpp does, which it includes.
#include "fbr_emul.cpp"

extern "C" {
// The producer tables of cut 0 / 1 (or of the forced cut points force[5] when force[0] >= 0), checked; returns 0, -1 when the model is
// outside the pass, or < -1 naming the check that failed.
// stats [4][6]: per part steps walked, owned links, owned entries, unowned links walked, entries of those, modelled cost (default coefficients).
// starts [5]: the cut points.  hash: a checksum of every table of the producer (the cut repeats).
int gram64_parts(const EmulTopo *t, int k, int cut, const int *force, double *stats, int *starts, unsigned long long *hash)
{
    FbrHostModel hm;
    make(t, hm);
    FbrGramProgram gp;
    fbr_gram_build_best(gp, hm, k, g_shape, !fbr_gram_rhs_moments(hm, k));
    FbrGram64 g;
    if (k > 1 || !fbr_gram64_build(hm, gp, g, true, false, 1)) return -1;
    FbrGram64Producer pr;
    std::vector<int> fs;
    if (force && force[0] >= 0) fs.assign(force, force + FBR_KINWRITE_PARTS + 1);
    if (!fbr_gram64_build_producer(hm, g, pr, cut, k, fs.empty() ? nullptr : &fs)) return -1;
    const int L = hm.L, NP = pr.nparts;
    if ((int)pr.starts.size() != NP + 1) return -2;
    // every column that has a tile has exactly one owning part, every other column none
    std::vector<int> has_tile(hm.cols, 0), owners(hm.cols, 0), ncol(L, 0), nfr(L, 0);
    for (int i = 0; i < g.NT; i++)
        for (int sl = 0; sl < FBR_TILE; sl++)
            if (g.tiles[i].col[sl] >= 0 && g.tiles[i].col[sl] < hm.cols) has_tile[g.tiles[i].col[sl]] = 1;
    for (int pq = 0; pq < NP; pq++)
        for (int l = 0; l < L; l++) {
            for (int p = 0; p < 10; p++) {
                const int c = pr.lcol[((size_t)pq * L + l) * 10 + p];
                if (c < 0) continue;
                if (c >= hm.ninert || hm.coldesc[c].link != l || hm.coldesc[c].pidx != p) return -3;
                if (!pr.rel[((size_t)pq * L + l) * FBR_G64_WORDS + p]) return -3;
                owners[c]++;
                ncol[l]++;
            }
            for (int p = 0; p < FBR_G64_FRIC; p++) {
                const int c = pr.lcol[(size_t)NP * 10 * L + ((size_t)pq * L + l) * FBR_G64_FRIC + p];
                if (c < 0) continue;
                if (c < hm.ninert || c >= hm.cols || hm.coldesc[c].joint != hm.dof[l]) return -3;
                if (!pr.rel[((size_t)pq * L + l) * FBR_G64_WORDS + 14 + p]) return -3;
                owners[c]++;
                nfr[l]++;
            }
        }
    for (int c = 0; c < hm.cols; c++)
        if (owners[c] != has_tile[c]) return -4;
    // a part's walked set: closed under parents, and it holds every link the part writes a column of
    const std::vector<int> lanecol = fbr_gram64_lane_columns(pr, L);
    for (int pq = 0; pq < NP; pq++) {
        std::vector<char> walked(L, 0);
        for (int s = 0; s < pr.nsteps[pq]; s++) {
            const int l = pr.steps[(size_t)(pr.step0[pq] + s) * FBR_KINID_STEP];
            if (l < 0 || l >= L || walked[l]) return -5;
            if (hm.parent[l] >= 0 && !walked[hm.parent[l]]) return -5;  // (the parent comes first)
            walked[l] = 1;
        }
        for (int l = 0; l < L; l++) {
            // the owns-nothing flag: exactly where all 18 words are zero and all lane columns are -1
            bool words = false, lanes = false;
            for (int i = 0; i < FBR_G64_WORDS; i++) words |= pr.rel[((size_t)pq * L + l) * FBR_G64_WORDS + i] != 0;
            for (int i = 0; i < 64; i++) lanes |= lanecol[((size_t)pq * L + l) * 64 + i] != -1;
            if (words != lanes) return -6;
            if (pr.none[(size_t)pq * L + l] != (words ? 0 : 1)) return -6;
            // a link the producer does not skip is one it walks: the image of emul_gram64, built from the words alone, is what a
            // producer writes that visits no flagged link
            if (words && !walked[l]) return -7;
            // ownership is by contiguous ranges of the depth-first order
            bool in_range = false;
            for (int i = pr.starts[pq]; i < pr.starts[pq + 1]; i++) in_range |= hm.order[i] == l;
            if (words && !in_range) return -8;
            if (in_range && !walked[l]) return -8;
        }
    }
    const std::vector<FbrGram64PartStats> st = fbr_gram64_part_stats(hm, ncol, nfr, pr.starts, k, FbrGram64PartModel());
    for (int pq = 0; pq < NP; pq++) {
        if (st[pq].steps != pr.nsteps[pq]) return -9;
        const double row[6] = {(double)st[pq].steps, (double)st[pq].links, (double)st[pq].entries, (double)st[pq].unowned, (double)st[pq].discarded, st[pq].cost};
        std::copy(row, row + 6, stats + 6 * pq);
    }
    for (int pq = NP; pq < FBR_KINWRITE_PARTS; pq++) std::fill(stats + 6 * pq, stats + 6 * pq + 6, 0.0);
    std::fill(starts, starts + FBR_KINWRITE_PARTS + 1, L);
    std::copy(pr.starts.begin(), pr.starts.end(), starts);
    unsigned long long h = 1469598103934665603ULL;
    auto mix = [&](long long v) { h = (h ^ (unsigned long long)v) * 1099511628211ULL; };
    for (long long v : pr.rel) mix(v);
    for (int v : pr.lcol) mix(v);
    for (int v : pr.steps) mix(v);
    for (int v : pr.none) mix(v);
    for (int v : pr.starts) mix(v);
    *hash = h;
    return NP;
}

// out: blocks of every chunk but the last, what the last may hold, chunks, Gram rounds, producer rounds, the largest chunk
int gram64_chunk_plan(long nblocks, long cap, long num_cus, long pgrid_max, int rule, long *out)
{
    if (cap < num_cus || nblocks <= cap) return -1;
    const FbrGram64ChunkPlan p = fbr_gram64_chunk_plan(nblocks, cap, num_cus, pgrid_max, rule);
    long largest = 0, n = 0;
    for (long left = nblocks; left > 0; n++) {
        const long nb = left <= p.last_cap ? left : p.chb;
        if (left > p.last_cap && p.chb % num_cus) return -2;  // (every chunk but the last: whole rounds of the Gram grid)
        largest = std::max(largest, nb);
        left -= nb;
    }
    if (n != p.chunks) return -3;
    const long o[6] = {p.chb, p.last_cap, p.chunks, p.gram_rounds, p.prod_rounds, largest};
    std::copy(o, o + 6, out);
    return 0;
}
}
