// gram64_runs.cpp -- the host tables of the Gram kernel's pipelined slot walk (csrc/fbr_gram64.h FbrGram64::runs), for
// tests/test_gram64_runs.py (TEST ONLY).  It builds the tables exactly as emul_gram64 of fbr_emul.cpp does, which it includes.
#include "fbr_emul.cpp"

extern "C" {
// dims: waves, slots per wave, levels, tiles (main + force), runs present (0 / 1).  wmeta [waves][slots][3] and runs [waves][levels] are
// written when cap (ints) holds them.  Returns < 0 when the model is outside the pass.
int gram64_runs(const EmulTopo *t, int k, int force_tiles, int *dims, int *wmeta, int *runs, long cap)
{
    FbrHostModel hm;
    make(t, hm);
    FbrGramProgram gp;
    fbr_gram_build_best(gp, hm, k, g_shape, !fbr_gram_rhs_moments(hm, k));
    FbrGram64 g;
    if (k > 1 || !fbr_gram64_build(hm, gp, g, force_tiles != 0, false)) return -1;
    dims[0] = g.wpb;
    dims[1] = g.npw;
    dims[2] = g.nlev;
    dims[3] = g.NT + g.NF;
    dims[4] = g.runs.empty() ? 0 : 1;
    if ((long)g.wmeta.size() > cap || (long)g.runs.size() > cap) return -2;
    std::copy(g.wmeta.begin(), g.wmeta.end(), wmeta);
    std::copy(g.runs.begin(), g.runs.end(), runs);
    return 0;
}
}
