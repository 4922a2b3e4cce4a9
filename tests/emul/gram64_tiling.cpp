// gram64_tiling.cpp -- the column tiles of the sample-contiguous Gram pass (csrc/fbr_gram64.h fbr_gram64_build, option gram_lane_tiling),
// for tests/test_gram64_tiling.py (TEST ONLY).  It builds the program exactly as emul_gram64 of fbr_emul.cpp does, which it includes.
#include "fbr_emul.cpp"

extern "C" {
// stats: tiling used, MFMAs per block, tile rows, main tiles, force tiles, pairs, busiest, balanced, stages, widest stage (slabs), LDS
// bytes, runs table present (0 / 1).  tiles [NT][16 columns | path length | 32 joints of the path] when cap (ints) holds them.
// Returns < 0 when the model is outside the pass.
int gram64_tiling(const EmulTopo *t, int k, int force_tiles, int tiling, long *stats, int *tiles, long cap)
{
    FbrHostModel hm;
    make(t, hm);
    FbrGramProgram gp;
    fbr_gram_build_best(gp, hm, k, g_shape, !fbr_gram_rhs_moments(hm, k));
    FbrGram64 g;
    if (k > 1 || !fbr_gram64_build(hm, gp, g, force_tiles != 0, false, tiling)) return -1;
    long npairs = 0;
    for (size_t i = 0; i < g.wmeta.size(); i += 3) npairs += g.wmeta[i] >= 0;
    const long st[12] = {g.tiling, g.mfma_per_block, g.ntr, g.NT, g.NF, npairs, g.busiest, g.balanced, g.nstage, g.maxact,
                         (long)fbr_gram64_lds_bytes(g), g.runs.empty() ? 0L : 1L};
    std::copy(st, st + 12, stats);
    if ((long)g.NT * 49 > cap) return -2;
    for (int i = 0; i < g.NT; i++) {
        int *o = tiles + (size_t)i * 49;
        std::copy(g.tiles[i].col, g.tiles[i].col + FBR_TILE, o);
        if (g.tiles[i].path.size() > 32) return -2;
        o[16] = (int)g.tiles[i].path.size();
        std::fill(o + 17, o + 49, -1);
        std::copy(g.tiles[i].path.begin(), g.tiles[i].path.end(), o + 17);
    }
    FbrGram64Producer pr;
    return fbr_gram64_build_producer(hm, g, pr) ? 0 : -3;
}

// per column: its link's joint path (length, then up to 32 joints) and its kind (0 inertial, 1 friction)
int gram64_colpaths(const EmulTopo *t, int *out, long cap)
{
    FbrHostModel hm;
    make(t, hm);
    if ((long)hm.cols * 34 > cap) return -2;
    for (int c = 0; c < hm.cols; c++) {
        int *o = out + (size_t)c * 34;
        std::fill(o, o + 34, -1);
        o[0] = hm.coldesc[c].kind;
        if (hm.coldesc[c].kind != 0) continue;
        const std::vector<int> &p = hm.path[hm.coldesc[c].link];
        if (p.size() > 32) return -2;
        o[1] = (int)p.size();
        std::copy(p.begin(), p.end(), o + 2);
    }
    return hm.cols;
}
}
