// fbr_gram64.h -- the fused Gram over SAMPLE-CONTIGUOUS images (round 6, option "gram_lane").
//
// The contraction G_ab = sum_s sum_r Y_s[r, a] Y_s[r, b] does not care in which order (s, r) is walked.  The first fused pass
// (fbr_kernels.h K5a / K5b) takes ONE sample's image per LDS-DMA and runs the MFMA k-steps over four ROWS of that sample: its producer has to
// lay out a sample's 20 KB contiguously, which a one-lane-per-sample producer can only do with 8-byte stores at a 33 KB stride (partially
// written lines) -- hence the record round trip kinematics kernel -> HBM -> workgroup-per-sample packer, which bounds that pass.
// Here the k-steps run over four SAMPLES of one regressor row:
//   * image of a block of 64 samples: [tile row tr][half][16 columns][32 samples], tile row = (column tile, real row of the tile: the fb
//     base-wrench rows, then the joints of the tile's path); no row padding, no paired base rows.  Inside a 32-sample run sample s of
//     column slot c sits at s ^ 2 c: an operand read of the MFMAs (lane (kk, li) -> column li, sample 4 ks + kk) is served half a wave at a
//     time, and the 32 lanes of a half (16 columns x two values of kk) then fall on the 32 different bank pairs of the LDS (with s ^ 4 (c & 7),
//     round 6's first layout, columns c and c + 8 collided: SQ_LDS_BANK_CONFLICT 42 % of the LDS cycles of the kernel), with the LDS layout
//     EQUAL to the global one (one contiguous 4 KB DMA per slab);
//   * producer fbr_kinimg_kernel: one lane per sample, kinematics fused in, the tree cut into parts for the waves of a workgroup
//     (fbr_kinid.h); every value of a (column, row) goes out as two 256-byte runs per wave;  the rhs columns' products with the columns (k <= 2) are
//     accumulated on the way: one six-term dot product per (column, rhs column) against the link's t_base + sum_j S_j t_j, added to the lane's own running
//     sum in HBM (no-return atomics, one adder per address: deterministic);
//   * consumer fbr_gram64_kernel: one workgroup of 8 waves per CU, the accumulators of the tile pairs in registers for the whole pass;
//     a stage = (a few consecutive row levels, 32 samples): the slabs of the tiles that have the levels arrive by LDS-DMA into one of two
//     buffers while the MFMAs of the stage before run; a pair takes part in the levels of its range; 8 MFMAs per pair, level and half block;
//   * the force rows of the base wrench (levels 0 .. 2) run on tiles of their own that hold the columns with a force only (fbr_gram64_build);
//   * the main tiles are the pass's own (fbr_gram64_fill_tiles): a column sits in any tile whose joint path contains its own.
// Conditions (else the first pass runs): k <= 2 rhs columns (or none), a tile program in one part; sample groups (fbr_gram_grouped) for k = 0.
// Friction columns are tiles whose levels are the rows of their own joints.
// Inputs resident in HBM or pinned host memory (staged chunk by chunk); row weights; a base-wrench-only row mask runs the base stages only.
#pragma once
// the swizzle of column slot c inside its 32-sample run (see the image layout above)
#define FBR_G64_SWZ(c) (2 * ((c) & 15))
#include <algorithm>
#include <type_traits>
#include <utility>

#include "fbr_kinid.h"

struct FbrGram64Tile {     // a main tile of the pass
    int col[FBR_TILE];     // column of each slot, -1 = padding
    std::vector<int> path; // joints of its rows: the path of each of its columns is a prefix of it
    int friction = 0;      // friction columns: the rows of their own joints only
    int lo = 0, hi = 0;    // its levels [lo, hi) (fbr_gram64_build)
};

struct FbrGram64 {  // host program
    int NT = 0;      // main tiles (tiles below)
    int NF = 0;      // force tiles (below); tiles are numbered main 0 .. NT-1, force NT .. NT+NF-1
    int nlev = 0, fb = 0, flev = 0, ntr = 0, maxact = 0, npw = 0, wpb = 8;  // npw accumulators per wave, wpb waves per workgroup (8 or 16)
    long blk_doubles = 0;
    std::vector<int> trow;       // [NT + NF][nlev] tile-row index or -1
    std::vector<int> slab;       // [nlev][NT + NF] slab index inside the level's stage or -1
    int nstage = 0, base_stages = 0;
    std::vector<int> stage_lev;  // [nstage + 1] first level of each stage
    std::vector<int> lev_begin;  // [nlev + 1] into pieces
    std::vector<int> pieces;     // pairs: global offset (doubles, inside the block image, half 0), LDS offset (doubles, inside a stage buffer)
    std::vector<int> wmeta;      // [wpb waves][npw][3]: tile I (-1: empty slot), tile J, first level | (one past the last level) << 8
    std::vector<int> runs;       // [wpb waves][nlev]: qa | qb << 8, the wave's slots active at the level are exactly qa .. qb-1 (empty table:
                                 // some wave's pairs admit no such order, and the kernel walks every slot at every level)
    std::vector<int> slot_tiles; // [2][wpb * npw * 2] for the two reductions: main pairs, force pairs (the other kind's slots are -1), in the
                                 // partial-sum order fbr_gram_reduce_kernel walks: [wave & 7][wave >> 3][slot] (16 waves = 8 rows of twice the slots)
    std::vector<int> tilecol;    // [NT + NF][16] column of each tile slot, -1 = padding
    std::vector<int> fcol_tile, fcol_slot;  // per column: its force tile / slot there, or -1
    std::vector<int> tile_lo;    // [NT] first level of every main / friction tile
    std::vector<FbrGram64Tile> tiles;  // [NT] the main tiles (fbr_gram64_build)
    int tiling = 0;                    // which tiling they are: 0 the tile program's, 1 the bottom-up fill (fbr_gram64_build)
    long mfma_per_block = 0;
    long busiest = 0, balanced = 0;  // sum over the stages of the busiest wave's pair-levels / of ceil(all pair-levels / 8)
};

// Levels [lo, hi) of a main tile before the force levels are known: a main tile has the base-wrench rows and the joints of its path; a
// FRICTION tile (its columns are non-zero on the row of their own joint only) just the levels of its own columns' joints -- a contiguous
// stretch of its path.  false: a friction tile without such a joint.
static inline bool fbr_gram64_tile_levels(const FbrHostModel &hm, FbrGram64Tile &t)
{
    t.lo = 0;
    t.hi = hm.fb + (int)t.path.size();
    if (!t.friction) return true;
    int jmin = (int)t.path.size(), jmax = -1;
    for (int sl = 0; sl < FBR_TILE; sl++) {
        if (t.col[sl] < 0) continue;
        const int jnt = hm.coldesc[t.col[sl]].joint;
        for (int j = 0; j < (int)t.path.size(); j++)
            if (t.path[j] == jnt) jmin = std::min(jmin, j), jmax = std::max(jmax, j);
    }
    if (jmax < 0) return false;
    t.lo = hm.fb + jmin;
    t.hi = hm.fb + jmax + 1;
    return true;
}

// ---- Tilings of the pass.  A pair of main tiles costs 16 MFMAs per block for every level it runs (moment levels + common prefix of the
// two paths), so the tiles that suit this pass are not the tile program's (built for the per-sample-image pass: tiles closed where a
// depth-first walk stops nesting, fewest tiles).  Any column can sit in a tile whose path contains its own: the base link, the waist and
// the upper links of a chain can fill up the tiles of deeper links, where a tile of their own would run levels against every other tile.
// The program's tiles as they are.  false: a tile outside this pass (dense).
static inline bool fbr_gram64_program_tiles(const FbrHostModel &hm, const FbrGramProgram &gp, std::vector<FbrGram64Tile> &tiles)
{
    tiles.assign(gp.NT, FbrGram64Tile());
    for (int t = 0; t < gp.NT; t++) {
        const FbrTile &tl = gp.tiles[t];
        if (tl.type != 0) return false;
        std::copy(tl.col, tl.col + FBR_TILE, tiles[t].col);
        tiles[t].path = tl.tpath;
        tiles[t].friction = tl.friction;
        if (!fbr_gram64_tile_levels(hm, tiles[t])) return false;
    }
    return true;
}

// Bottom-up fill of the inertial columns of `from` (friction tiles kept as they are, behind): the deepest unplaced column opens a tile on
// its path, which takes the unplaced columns nested in that path, deepest first (ties: column order), until it is full; repeat.
static inline void fbr_gram64_fill_tiles(const FbrHostModel &hm, const std::vector<FbrGram64Tile> &from, std::vector<FbrGram64Tile> &tiles)
{
    std::vector<int> cols;
    for (const FbrGram64Tile &t : from)
        if (!t.friction)
            for (int c : t.col)
                if (c >= 0) cols.push_back(c);
    auto depth = [&](int c) { return (int)hm.path[hm.coldesc[c].link].size(); };
    std::stable_sort(cols.begin(), cols.end(), [&](int x, int y) { return depth(x) != depth(y) ? depth(x) > depth(y) : x < y; });
    std::vector<char> placed(cols.size(), 0);
    tiles.clear();
    for (size_t i = 0; i < cols.size(); i++) {
        if (placed[i]) continue;
        FbrGram64Tile t;
        std::fill(t.col, t.col + FBR_TILE, -1);
        t.path = hm.path[hm.coldesc[cols[i]].link];
        for (size_t j = i, fill = 0; j < cols.size() && fill < FBR_TILE; j++)
            if (!placed[j] && FbrGramProgram::nested(t.path, hm.path[hm.coldesc[cols[j]].link])) {
                t.col[fill++] = cols[j];
                placed[j] = 1;
            }
        fbr_gram64_tile_levels(hm, t);
        tiles.push_back(t);
    }
    for (const FbrGram64Tile &t : from)
        if (t.friction) tiles.push_back(t);
}

// Tiles / pairs of the pass for the given main tiles; pairs: (I, J) of every main pair in slot order, or empty: every I <= J that runs
// at least one level.
//
// FORCE TILES (floating base).  The first three regressor rows are the force rows of the base wrench, and only the mass and the first
// moments of a link produce a force: in the column tiles of the program most entries of those rows are structural zeros (6 of 10 columns
// of a full link, 5 of 7 of a regrouped one), yet every tile pair pays three levels for them -- a third of all MFMAs of WALK-MAN.  So the
// force rows get tiles of their own: the columns that have a force, 16 to a tile in column order (base rows are common to all columns:
// no path condition), every pair of force tiles runs levels 0 .. 2, and the program's tiles start at level 3.  An entry G_ab with two
// force columns is the sum of its two blocks (two reductions, one after the other).  Used when the extra pairs fit the accumulator slots.
// wide16 (option gram_lane_waves = 16): models of the one-workgroup-per-CU shape (18 accumulators per wave of an 8-wave workgroup) run 16
// waves of 10 accumulators instead -- four waves per SIMD at 128 registers.  Measured: the Gram kernel 9.70 instead of 9.32 ms per 1 M
// WALK-MAN samples (operand reads in half groups, more A reloads, less reuse per wave): not the default.
static inline bool fbr_gram64_build_tiles(const FbrHostModel &hm, const FbrGramConfig &cfg, const std::vector<FbrGram64Tile> &tiles,
                                          const std::vector<int> &pairs, FbrGram64 &g, bool force_tiles, bool wide16)
{
    g.npw = cfg.segw * cfg.nseg;
    g.wpb = FBR_WPB;
    if (wide16 && g.npw > 10) {
        g.wpb = 2 * FBR_WPB;
        g.npw = 10;
    }
    const int W = g.wpb;
    g.tiles = tiles;
    g.NT = (int)tiles.size();
    g.fb = hm.fb;
    g.nlev = 0;
    std::vector<int> tlo(g.NT, 0), thi(g.NT, 0);
    for (int t = 0; t < g.NT; t++) {
        tlo[t] = tiles[t].lo;
        thi[t] = tiles[t].hi;
        if (thi[t] <= tlo[t]) return false;  // (a tile without rows: the columns of the base link of a fixed base)
        g.nlev = std::max(g.nlev, thi[t]);
    }
    if (g.nlev == 0 || g.nlev > 255) return false;
    // the tile pairs: unordered, with their common depth cp = fb + joints both tiles' columns have rows on
    struct Pr {
        int a, b, lo, hi;
    };
    std::vector<Pr> prs;
    auto add = [&](int I, int J) {
        const int cp = hm.fb + FbrGramProgram::common_prefix(tiles[I].path, tiles[J].path);
        prs.push_back({I, J, std::max(tlo[I], tlo[J]), std::min(cp, std::min(thi[I], thi[J]))});
    };
    for (size_t i = 0; i + 1 < pairs.size(); i += 2) add(pairs[i], pairs[i + 1]);
    if (pairs.empty())
        for (int I = 0; I < g.NT; I++)
            for (int J = I; J < g.NT; J++) {
                add(I, J);
                if (prs.back().lo >= prs.back().hi) prs.pop_back();
            }
    // force columns and their tiles
    g.fcol_tile.assign(hm.cols, -1);
    g.fcol_slot.assign(hm.cols, -1);
    g.tilecol.assign((size_t)g.NT * FBR_TILE, -1);
    std::vector<char> has_tile(hm.cols, 0);
    for (int t = 0; t < g.NT; t++)
        for (int sl = 0; sl < FBR_TILE; sl++) {
            const int c = tiles[t].col[sl];
            if (c >= 0 && c < hm.cols) {
                if (has_tile[c]) return false;
                g.tilecol[(size_t)t * FBR_TILE + sl] = c;
                has_tile[c] = 1;
            }
        }
    g.NF = 0;
    g.flev = 0;
    if (force_tiles && hm.fb == 6) {
        int nf = 0;
        for (int c = 0; c < hm.ninert; c++)
            if (has_tile[c] && hm.coldesc[c].pidx < 4) {
                g.fcol_tile[c] = g.NT + nf / FBR_TILE;
                g.fcol_slot[c] = nf % FBR_TILE;
                nf++;
            }
        const int NF = (nf + FBR_TILE - 1) / FBR_TILE;
        if (NF > 0 && (long)prs.size() + (long)NF * (NF + 1) / 2 <= (long)W * g.npw) {
            g.NF = NF;
            g.flev = 3;
        } else {
            std::fill(g.fcol_tile.begin(), g.fcol_tile.end(), -1);
            std::fill(g.fcol_slot.begin(), g.fcol_slot.end(), -1);
        }
    }
    const int NTT = g.NT + g.NF;
    g.tilecol.resize((size_t)NTT * FBR_TILE, -1);
    for (int c = 0; c < hm.cols; c++)
        if (g.fcol_tile[c] >= 0) g.tilecol[(size_t)g.fcol_tile[c] * FBR_TILE + g.fcol_slot[c]] = c;
    for (int t = 0; t < g.NT; t++)
        if (!tiles[t].friction) g.tiles[t].lo = tlo[t] = g.flev;  // (the main tiles start behind the force levels)
    for (Pr &p : prs) p.lo = std::max(p.lo, std::max(tlo[p.a], tlo[p.b]));
    prs.erase(std::remove_if(prs.begin(), prs.end(), [](const Pr &p) { return p.lo >= p.hi; }), prs.end());
    for (int f = 0; f < g.NF; f++)
        for (int f2 = f; f2 < g.NF; f2++) prs.push_back({g.NT + f, g.NT + f2, 0, g.flev});
    // tile rows: the force tiles' first (so that "level 0" of a main tile, flev rows in front of its first row, is inside the image), then the
    // rows of every main tile one after the other -- the producer relies on consecutive rows: level lv of a column sits 1024 doubles x lv
    // behind its level 0
    g.trow.assign((size_t)NTT * g.nlev, -1);
    g.ntr = 0;
    for (int f = 0; f < g.NF; f++)
        for (int lv = 0; lv < g.flev; lv++) g.trow[(size_t)(g.NT + f) * g.nlev + lv] = g.ntr++;
    for (int t = 0; t < g.NT; t++) {
        g.ntr = std::max(g.ntr, tlo[t]);  // ("level 0" of the tile, tlo rows in front of its first one, must not fall in front of the image)
        for (int lv = tlo[t]; lv < thi[t]; lv++) g.trow[(size_t)t * g.nlev + lv] = g.ntr++;
    }
    g.tile_lo = tlo;
    g.blk_doubles = (long)g.ntr * 1024;
    // Stages: consecutive levels whose slabs fit one LDS buffer together share a stage --
    // one barrier and one round of LDS-DMA for the three force levels, or for the deep levels only a few tiles reach.
    std::vector<int> nslab(g.nlev, 0);
    int widest = 0;
    for (int lv = 0; lv < g.nlev; lv++) {
        for (int t = 0; t < NTT; t++) nslab[lv] += g.trow[(size_t)t * g.nlev + lv] >= 0;
        widest = std::max(widest, nslab[lv]);
    }
    // (the two-per-CU shape of small models keeps its workgroups below half the LDS: 2 buffers x 8 slabs x 4 KB)
    const int cap = std::max(widest, g.npw <= 10 ? 8 : 16);
    g.stage_lev.assign(1, 0);
    for (int lv = 0, in_stage = 0; lv < g.nlev; lv++) {
        if (lv > g.stage_lev.back() && (in_stage + nslab[lv] > cap || lv == hm.fb)) {  // (the base-wrench rows end a stage: base_stages)
            g.stage_lev.push_back(lv);
            in_stage = 0;
        }
        in_stage += nslab[lv];
    }
    g.stage_lev.push_back(g.nlev);
    g.nstage = (int)g.stage_lev.size() - 1;
    if (g.nstage > 62) return false;  // (the kernel keeps the stages' constants one per lane)
    g.base_stages = 0;  // stages of the base-wrench rows alone: all a call runs whose row weights switch every joint row off
    while (g.base_stages < g.nstage && g.stage_lev[g.base_stages + 1] <= hm.fb) g.base_stages++;
    g.slab.assign((size_t)g.nlev * NTT, -1);
    g.lev_begin.assign(g.nlev + 1, 0);
    g.pieces.clear();
    g.maxact = 0;
    for (int sg = 0; sg < g.nstage; sg++) {
        int idx = 0;
        for (int lv = g.stage_lev[sg]; lv < g.stage_lev[sg + 1]; lv++) {
            g.lev_begin[lv] = (int)g.pieces.size() / 2;
            for (int t = 0; t < NTT; t++) {
                const int tr = g.trow[(size_t)t * g.nlev + lv];
                if (tr < 0) continue;
                g.slab[(size_t)lv * NTT + t] = idx;
                for (int p = 0; p < 4; p++) {
                    g.pieces.push_back(tr * 1024 + p * 128);
                    g.pieces.push_back(idx * 512 + p * 128);
                }
                idx++;
            }
        }
        g.maxact = std::max(g.maxact, idx);
    }
    g.lev_begin[g.nlev] = (int)g.pieces.size() / 2;
    // Pairs -> waves.  All waves of the workgroup meet at every stage (level, half block), so a stage lasts as long as its busiest wave: the
    // cost of a placement is  sum over levels of max over waves of the pairs active at the level,  not the waves' totals (the tile program's
    // own placement, balanced by totals, leaves WALK-MAN at 156 against 126 for a perfect split).  Any pair may sit in any accumulator of
    // any wave (the kernel reloads the A operand when the tile I of the next slot differs).  Deal by decreasing length, then local search:
    // move a pair / swap two while (cost, sum of squared loads) falls.  Deterministic.
    const int NP = (int)prs.size();
    if (NP > W * g.npw) return false;
    std::vector<int> order(NP), wave_of(NP, -1), cnt(W, 0);
    for (int i = 0; i < NP; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return prs[x].hi - prs[x].lo > prs[y].hi - prs[y].lo; });
    std::vector<std::vector<int>> wl(W, std::vector<int>(g.nlev, 0));
    auto shift = [&](int i, int w, int sign) {
        for (int lv = prs[i].lo; lv < prs[i].hi; lv++) wl[w][lv] += sign;
        cnt[w] += sign;
    };
    auto score = [&](long &c, long &sq) {  // (the waves meet once per stage: the loads of a stage's levels add up)
        c = 0, sq = 0;
        for (int sg = 0; sg < g.nstage; sg++) {
            int mx = 0;
            for (int w = 0; w < W; w++) {
                int tot = 0;
                for (int lv = g.stage_lev[sg]; lv < g.stage_lev[sg + 1]; lv++) tot += wl[w][lv];
                mx = std::max(mx, tot);
                sq += (long)tot * tot;
            }
            c += mx;
        }
    };
    for (int r = 0; r < NP; r++) {  // snake deal
        const int round = r / W, pos = r % W, w = (round & 1) ? W - 1 - pos : pos;
        wave_of[order[r]] = w;
        shift(order[r], w, +1);
    }
    long c0, q0;
    score(c0, q0);
    for (int sweep = 0, improved = 1; improved && sweep < 64; sweep++) {
        improved = 0;
        for (int i = 0; i < NP; i++) {
            for (int w2 = 0; w2 < W; w2++) {
                const int w1 = wave_of[i];
                if (w2 == w1 || cnt[w2] >= g.npw) continue;
                shift(i, w1, -1), shift(i, w2, +1);
                long c1, q1;
                score(c1, q1);
                if (c1 < c0 || (c1 == c0 && q1 < q0)) {
                    wave_of[i] = w2, c0 = c1, q0 = q1, improved = 1;
                } else {
                    shift(i, w2, -1), shift(i, w1, +1);
                }
            }
            for (int k2 = i + 1; k2 < NP; k2++) {
                const int w1 = wave_of[i], w2 = wave_of[k2];
                if (w1 == w2 || (prs[i].lo == prs[k2].lo && prs[i].hi == prs[k2].hi)) continue;
                shift(i, w1, -1), shift(k2, w2, -1), shift(i, w2, +1), shift(k2, w1, +1);
                long c1, q1;
                score(c1, q1);
                if (c1 < c0 || (c1 == c0 && q1 < q0)) {
                    wave_of[i] = w2, wave_of[k2] = w1, c0 = c1, q0 = q1, improved = 1;
                } else {
                    shift(i, w2, -1), shift(k2, w1, -1), shift(i, w1, +1), shift(k2, w2, +1);
                }
            }
        }
    }
    g.busiest = c0;
    g.balanced = 0;
    for (int sg = 0; sg < g.nstage; sg++) {
        int tot = 0;
        for (int lv = g.stage_lev[sg]; lv < g.stage_lev[sg + 1]; lv++)
            for (int w = 0; w < W; w++) tot += wl[w][lv];
        g.balanced += (tot + W - 1) / W;
    }
    // slots of a wave: the A operand (tile I) of a slot is kept for the next one when it is the same tile, so the pairs of a wave are ordered
    // by the tile most of them contain (which of a pair's two tiles is "I" is free: the reduction writes the block and its mirror image)
    // Runs (the 8 x 18 shape): the kernel pipelines a level's active slots -- the operand reads of the next one in flight while the MFMAs of
    // the current one run -- when they are consecutive slots.  The force pairs (levels 0 .. flev-1) first, then the others by end level,
    // descending: the main pairs all start at flev, so the active ones of a level are a prefix of them.  Friction pairs start later and may
    // break that; the run table stays empty then.  Ties keep the order above (same tile I next to each other: the A operand is kept).
    // Neither the roles of a pair's tiles nor the order of its MFMAs change: only which slot holds it.
    std::vector<std::vector<int>> slots(W);  // per wave: pairs, each with its tile I in front (T, J, lo, hi)
    for (int w = 0; w < W; w++) {
        std::vector<int> mine;
        for (int i = 0; i < NP; i++)
            if (wave_of[i] == w) mine.push_back(i);
        std::vector<char> done(NP, 0);
        for (size_t left = mine.size(); left > 0;) {
            std::vector<int> freq(NTT, 0);
            for (int i : mine)
                if (!done[i]) {
                    freq[prs[i].a]++;
                    if (prs[i].b != prs[i].a) freq[prs[i].b]++;
                }
            int T = 0;
            for (int t = 1; t < NTT; t++)
                if (freq[t] > freq[T]) T = t;
            for (int i : mine) {
                if (done[i] || (prs[i].a != T && prs[i].b != T)) continue;
                const int J = prs[i].a == T ? prs[i].b : prs[i].a;
                slots[w].insert(slots[w].end(), {T, J, prs[i].lo, prs[i].hi});
                done[i] = 1;
                left--;
            }
        }
    }
    g.runs.clear();
    if (W == 8 && g.npw > 10) {
        std::vector<std::vector<int>> sorted(W);
        std::vector<int> runs((size_t)W * g.nlev, 0);
        bool ok = true;
        for (int w = 0; w < W && ok; w++) {
            const int n = (int)slots[w].size() / 4;
            std::vector<int> ord(n);
            for (int q = 0; q < n; q++) ord[q] = q;
            const int *sw = slots[w].data();
            std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) {
                const bool fx = sw[4 * x] >= g.NT, fy = sw[4 * y] >= g.NT;
                return fx != fy ? fx : sw[4 * x + 3] > sw[4 * y + 3];
            });
            for (int q : ord) sorted[w].insert(sorted[w].end(), sw + 4 * q, sw + 4 * q + 4);
            for (int lv = 0; lv < g.nlev && ok; lv++) {
                int qa = -1, qb = -1;
                for (int q = 0; q < n; q++) {
                    const bool act = sorted[w][4 * q + 2] <= lv && lv < sorted[w][4 * q + 3];
                    if (act && qa < 0) qa = q;
                    if (act && qb >= 0) ok = false;  // (an active slot behind an inactive one)
                    if (!act && qa >= 0 && qb < 0) qb = q;
                }
                if (qa < 0) qa = qb = 0;
                else if (qb < 0) qb = n;
                runs[(size_t)w * g.nlev + lv] = qa | (qb << 8);
            }
        }
        if (ok) {
            slots.swap(sorted);
            g.runs.swap(runs);
        }
    }
    g.wmeta.assign((size_t)W * g.npw * 3, -1);
    g.slot_tiles.assign((size_t)2 * W * g.npw * 2, -1);
    g.mfma_per_block = 0;
    for (int w = 0; w < W; w++)
        for (int q = 0; q < (int)slots[w].size() / 4; q++) {
            const int T = slots[w][4 * q], J = slots[w][4 * q + 1], lo = slots[w][4 * q + 2], hi = slots[w][4 * q + 3];
            const size_t s = (size_t)w * g.npw + q;                                       // wmeta: wave-major
            const size_t sr = ((size_t)(w & 7) * (W / 8) + (size_t)(w >> 3)) * g.npw + q;  // the reduction's order
            g.wmeta[3 * s] = T;
            g.wmeta[3 * s + 1] = J;
            g.wmeta[3 * s + 2] = lo | (hi << 8);
            const int kind = T >= g.NT ? 1 : 0;
            g.slot_tiles[((size_t)kind * W * g.npw + sr) * 2] = T;
            g.slot_tiles[((size_t)kind * W * g.npw + sr) * 2 + 1] = J;
            g.mfma_per_block += 16L * (hi - lo);  // 8 MFMAs per level and half
        }
    return true;
}

// LDS of fbr_gram64_kernel: two stage buffers, then the tables
#define FBR_G64_LDS_MAX (156 * 1024)
static inline size_t fbr_gram64_lds_bytes(const FbrGram64 &g)
{
    return (size_t)2 * g.maxact * 512 * sizeof(double) +
           ((size_t)g.nlev * (g.NT + g.NF) + g.nlev + 1 + g.pieces.size() + g.wmeta.size() + g.stage_lev.size() + g.runs.size()) * sizeof(int);
}

// The program of the pass for a one-part tile program built WITHOUT rhs tiles (moments); false: the model is outside this pass.
// tiling (option gram_lane_tiling) 0: the tile program's tiles and pairs.  1: the cheaper of those and the bottom-up fill -- by MFMAs per
// block (sum of pair-levels), then tile rows -- if the fill's program fits the kernel (pairs in the accumulator slots, stages, LDS): never
// more MFMAs than 0, and the pass serves the same models.
static inline bool fbr_gram64_build(const FbrHostModel &hm, const FbrGramProgram &gp, FbrGram64 &g, bool force_tiles = true, bool wide16 = false,
                                    int tiling = 1)
{
    if (gp.T != 1 || (gp.k > 0 && gp.rhs_tiles)) return false;
    std::vector<FbrGram64Tile> prog;
    if (!fbr_gram64_program_tiles(hm, gp, prog)) return false;
    std::vector<int> pairs;
    for (size_t s = 0; s < gp.slots.size(); s++) {
        const int pi = gp.slots[s].pair;
        if (pi < 0) continue;
        if (gp.pairs[pi].mode != 0) return false;
        pairs.insert(pairs.end(), {gp.pairs[pi].I, gp.pairs[pi].J});
    }
    bool ok = fbr_gram64_build_tiles(hm, gp.cfg, prog, pairs, g, force_tiles, wide16) && fbr_gram64_lds_bytes(g) <= FBR_G64_LDS_MAX;
    g.tiling = 0;
    if (!ok || !tiling) return ok;
    std::vector<FbrGram64Tile> fill;
    fbr_gram64_fill_tiles(hm, prog, fill);
    FbrGram64 c;
    if (fbr_gram64_build_tiles(hm, gp.cfg, fill, {}, c, force_tiles, wide16) && fbr_gram64_lds_bytes(c) <= FBR_G64_LDS_MAX &&
        (c.mfma_per_block < g.mfma_per_block || (c.mfma_per_block == g.mfma_per_block && c.ntr < g.ntr))) {
        g = std::move(c);
        g.tiling = 1;
    }
    return true;
}

// Producer tables: the tree in parts for the waves of a workgroup (fbr_kinid.h) and, per (part, link), 14 destination words: one per
// parameter, then the FORCE-tile words of parameters 0 .. 3.  A word: byte offset inside an image buffer of (level 0 of the column's tile
// rows, column slot, sample 0) -- a multiple of 256 -- with the slot's swizzle (FBR_G64_SWZ) in its low byte and bit 62 set (0: the part does not write that
// column).  Level lv of the column is 8192 bytes x lv further on (the tile rows of a tile are consecutive; with force tiles "level 0" of a
// main tile is three rows in front of its first row, rows 0 .. 2 of a force column go through its force word).
#define FBR_G64_WORDS 18  // 10 parameters, the force-tile words of parameters 0 .. 3, up to 4 friction columns of the link's joint
#define FBR_G64_FRIC 4
struct FbrGram64Producer {
    int nparts = 1, nslots = 1, step0[FBR_KINWRITE_PARTS] = {0, 0, 0, 0}, nsteps[FBR_KINWRITE_PARTS] = {0, 0, 0, 0};
    std::vector<long long> rel;  // [nparts][L][14]
    std::vector<int> lcol;       // [nparts][10 L] the column (for the rhs moments) or -1, then [nparts][4 L] the friction columns of the link's joint
    std::vector<int> steps;      // the parts' step programs, one after the other
    std::vector<int> none;       // [nparts][L] 1: the part writes no column of the link -- all 18 words zero, every lane column -1 (the producer skips the link's columns)
    std::vector<int> starts;     // [nparts + 1] part p owns positions [starts[p], starts[p + 1]) of the depth-first order
};

// What a part of the producer costs its wave per block, in fp64 instructions counted from the kernel's code (not fitted to launch times):
// a per step walked (the kinematic step: ancestors included), b per owned link (its column words, ten unit wrenches and moments),
// c per owned entry (one dot product, weight and store: an inertial column has fb + depth of them, a friction column one), d per owned
// entry more with rhs columns (the link's w^2 rhs vector, the columns' products with it and their sums over the wave).
struct FbrGram64PartModel {
    double a = 300.0, b = 400.0, c = 5.0, d = 1.0;
};
struct FbrGram64PartStats {
    int steps = 0, links = 0, entries = 0, unowned = 0, discarded = 0;  // discarded: the 10 (fb + depth) entries a producer without the skip forms for each unowned link it walks
    double cost = 0.0;
};
// the parts of cut points `starts` (fbr_kinid_build_parts_at) under model pm: ncol[l] inertial columns and nfr[l] friction columns written of link l
static inline std::vector<FbrGram64PartStats> fbr_gram64_part_stats(const FbrHostModel &hm, const std::vector<int> &ncol, const std::vector<int> &nfr,
                                                                    const std::vector<int> &starts, int k, const FbrGram64PartModel &pm)
{
    std::vector<FbrGram64PartStats> st(starts.size() - 1);
    for (size_t p = 0; p + 1 < starts.size(); p++) {
        std::vector<char> keep(hm.L, 0), mine(hm.L, 0);
        for (int i = starts[p]; i < starts[p + 1]; i++) {
            const int l = hm.order[i];
            mine[l] = 1;
            for (int a = l; a >= 0 && !keep[a]; a = hm.parent[a]) keep[a] = 1;
        }
        for (int l = 0; l < hm.L; l++) {
            if (!keep[l]) continue;
            const int e = ncol[l] * (hm.fb + (int)hm.path[l].size()) + nfr[l];
            st[p].steps++;
            if (mine[l]) {
                st[p].links++;
                st[p].entries += e;
            } else {
                st[p].unowned++;
                st[p].discarded += 10 * (hm.fb + (int)hm.path[l].size());
            }
        }
        st[p].cost = pm.a * st[p].steps + pm.b * st[p].links + (pm.c + (k > 0 ? pm.d : 0.0)) * st[p].entries;
    }
    return st;
}
// The cut that minimises the slowest part under pm, ancestors included: every choice of nparts contiguous ranges of the depth-first order
// is tried (a model has a few dozen links; above 256 links, or with fewer links than parts, `old` stays).  Ties stay with `old`, the cut
// fbr_kinid_build_parts made, then go to the cut nearest to it, then to the first one in the order of the search: the same cut every time.
static inline std::vector<int> fbr_gram64_cut_parts(const FbrHostModel &hm, const std::vector<int> &ncol, const std::vector<int> &nfr,
                                                    const std::vector<int> &old, int k, const FbrGram64PartModel &pm)
{
    const int L = hm.L, np = (int)old.size() - 1;
    if (np != FBR_KINWRITE_PARTS || L > 256 || L < np) return old;
    // cost of the range [i, j) as a part, for every i < j: links join one at a time, each bringing the ancestors not yet walked
    std::vector<double> rc((size_t)(L + 1) * (L + 1), 0.0);
    const double ce = pm.c + (k > 0 ? pm.d : 0.0);
    std::vector<char> keep(L);
    for (int i = 0; i < L; i++) {
        std::fill(keep.begin(), keep.end(), 0);
        double cost = 0.0;
        for (int j = i; j < L; j++) {
            const int l = hm.order[j];
            for (int a = l; a >= 0 && !keep[a]; a = hm.parent[a]) keep[a] = 1, cost += pm.a;
            cost += pm.b + ce * (ncol[l] * (hm.fb + (int)hm.path[l].size()) + nfr[l]);
            rc[(size_t)i * (L + 1) + j + 1] = cost;
        }
    }
    auto R = [&](int i, int j) { return rc[(size_t)i * (L + 1) + j]; };
    auto worst = [&](int c1, int c2, int c3) { return std::max(std::max(R(0, c1), R(c1, c2)), std::max(R(c2, c3), R(c3, L))); };
    int best[3] = {old[1], old[2], old[3]}, bestdist = 0;
    double bestmax = worst(old[1], old[2], old[3]);
    for (int c1 = 1; c1 < L - 2; c1++) {
        if (R(0, c1) > bestmax) break;  // (a range only grows dearer)
        for (int c2 = c1 + 1; c2 < L - 1; c2++) {
            if (R(c1, c2) > bestmax) break;
            for (int c3 = c2 + 1; c3 < L; c3++) {
                const double w = worst(c1, c2, c3);
                const int dist = std::abs(c1 - old[1]) + std::abs(c2 - old[2]) + std::abs(c3 - old[3]);
                if (w < bestmax || (w == bestmax && dist < bestdist)) {
                    bestmax = w;
                    bestdist = dist;
                    best[0] = c1, best[1] = c2, best[2] = c3;
                }
            }
        }
    }
    return {0, best[0], best[1], best[2], L};
}

// cut (option gram_lane_parts_cut) 0: the parts of fbr_kinid_build_parts (about equal cost of the OWNED links).  1: fbr_gram64_cut_parts.
// Which part writes a column changes neither the image nor any running sum.
static inline bool fbr_gram64_build_producer(const FbrHostModel &hm, const FbrGram64 &g, FbrGram64Producer &pr, int cut = 0, int k = 1,
                                             const std::vector<int> *force_starts = nullptr)
{
    std::vector<int> tile_of(hm.cols, -1), slot_of(hm.cols, -1);
    for (int t = 0; t < g.NT; t++)
        for (int sl = 0; sl < FBR_TILE; sl++)
            if (g.tiles[t].col[sl] >= 0 && g.tiles[t].col[sl] < hm.cols) {
                tile_of[g.tiles[t].col[sl]] = t;
                slot_of[g.tiles[t].col[sl]] = sl;
            }
    std::vector<double> lcost(hm.L, 30.0);
    for (int c = 0; c < hm.ninert; c++)
        if (tile_of[c] >= 0) lcost[hm.coldesc[c].link] += 10.0 + (double)(hm.fb + hm.path[hm.coldesc[c].link].size());
    std::vector<FbrKinIdProgram> progs;
    std::vector<std::vector<char>> own;
    try {
        fbr_kinid_build_parts(hm, lcost, FBR_KINWRITE_PARTS, progs, own);
        pr.starts = fbr_kinid_parts_starts(hm, own);
        if (cut || force_starts) {
            std::vector<int> ncol(hm.L, 0), nfr(hm.L, 0);
            for (int c = 0; c < hm.cols; c++) {
                if (tile_of[c] < 0) continue;
                if (c < hm.ninert) {
                    ncol[hm.coldesc[c].link]++;
                } else {
                    for (int x = 0; x < hm.L; x++)
                        if (hm.dof[x] == hm.coldesc[c].joint) nfr[x]++;
                }
            }
            const std::vector<int> starts = force_starts ? *force_starts : fbr_gram64_cut_parts(hm, ncol, nfr, pr.starts, k, FbrGram64PartModel());
            if (starts != pr.starts) {
                fbr_kinid_build_parts_at(hm, starts, progs, own);
                pr.starts = starts;
            }
        }
    } catch (const std::exception &) {
        return false;
    }
    pr.nparts = (int)progs.size();
    pr.rel.assign((size_t)pr.nparts * FBR_G64_WORDS * hm.L, 0);
    pr.lcol.assign((size_t)pr.nparts * (10 + FBR_G64_FRIC) * hm.L, -1);
    const int nfric = hm.n > 0 ? (hm.cols - hm.ninert) / hm.n : 0;
    if (nfric > FBR_G64_FRIC) return false;
    auto word = [](long long tile_row, int sl) { return ((tile_row * 1024 + sl * 32) * 8) | (long long)FBR_G64_SWZ(sl) | (1LL << 62); };
    for (int c = 0; c < hm.ninert; c++) {
        const int t = tile_of[c], sl = slot_of[c], l = hm.coldesc[c].link, pidx = hm.coldesc[c].pidx;
        if (t < 0) continue;  // (a column without a tile: structurally zero, e.g. the base link of a fixed base)
        if (!FbrGramProgram::nested(g.tiles[t].path, hm.path[l]) || hm.path[l].size() > g.tiles[t].path.size()) return false;  // (cannot happen: the tile's path contains the link's)
        const long long tr0 = (long long)g.trow[(size_t)t * g.nlev + g.tile_lo[t]] - g.tile_lo[t];
        if (tr0 < 0) return false;  // (cannot happen: the force tiles' rows come first)
        for (int pq = 0; pq < pr.nparts; pq++)
            if (own[pq][l]) {
                long long *w14 = &pr.rel[((size_t)pq * hm.L + l) * FBR_G64_WORDS];
                w14[pidx] = word(tr0, sl);
                if (g.fcol_tile[c] >= 0) {
                    if (pidx >= 4) return false;
                    w14[10 + pidx] = word(g.trow[(size_t)g.fcol_tile[c] * g.nlev], g.fcol_slot[c]);
                }
                pr.lcol[((size_t)pq * hm.L + l) * 10 + pidx] = c;
            }
    }
    // friction columns: the part that owns the joint's link writes them, on the row of that joint (level fb + position of the joint on the path)
    for (int c = hm.ninert; c < hm.cols; c++) {
        const int t = tile_of[c], sl = slot_of[c], d = hm.coldesc[c].joint, p = (c - hm.ninert) / std::max(hm.n, 1);
        if (t < 0) continue;
        int l = -1;
        for (int x = 0; x < hm.L; x++)
            if (hm.dof[x] == d) l = x;
        if (l < 0 || p >= FBR_G64_FRIC || hm.path[l].empty() || hm.path[l].back() != d) return false;
        const int lv = hm.fb + (int)hm.path[l].size() - 1;
        if (lv < g.tile_lo[t] || g.trow[(size_t)t * g.nlev + lv] < 0) return false;
        const long long tr0 = (long long)g.trow[(size_t)t * g.nlev + g.tile_lo[t]] - g.tile_lo[t];
        if (tr0 < 0) return false;
        for (int pq = 0; pq < pr.nparts; pq++)
            if (own[pq][l]) {
                pr.rel[((size_t)pq * hm.L + l) * FBR_G64_WORDS + 14 + p] = word(tr0, sl);
                pr.lcol[(size_t)pr.nparts * 10 * hm.L + ((size_t)pq * hm.L + l) * FBR_G64_FRIC + p] = c;
            }
    }
    pr.none.assign((size_t)pr.nparts * hm.L, 1);
    for (int pq = 0; pq < pr.nparts; pq++)
        for (int l = 0; l < hm.L; l++)
            for (int i = 0; i < FBR_G64_WORDS; i++)
                if (pr.rel[((size_t)pq * hm.L + l) * FBR_G64_WORDS + i]) pr.none[(size_t)pq * hm.L + l] = 0;
    pr.steps.clear();
    pr.nslots = 1;
    for (int pq = 0; pq < pr.nparts; pq++) {
        pr.step0[pq] = (int)(pr.steps.size() / FBR_KINID_STEP);
        pr.nsteps[pq] = progs[pq].nsteps;
        pr.nslots = std::max(pr.nslots, progs[pq].nslots);
        pr.steps.insert(pr.steps.end(), progs[pq].steps.begin(), progs[pq].steps.begin() + (size_t)progs[pq].nsteps * FBR_KINID_STEP);
    }
    return true;
}

// The chunks of a call of nblocks blocks that does not fit one chunk of `cap` blocks (cap >= num_cus): every chunk but the last has *chb
// blocks, a multiple of num_cus, and the last takes what is left once that is at most *last_cap.  The Gram kernel runs a chunk in rounds
// of num_cus workgroups, the producer in rounds of min(*chb, pgrid_max).
// rule (option gram_lane_chunk_rounds) 0: chunks as large as the cap allows, the last one no larger.  1: the fewest Gram rounds, then
// the fewest producer rounds, then the fewest chunks, then the largest chunks; the last chunk may be the largest (at most cap).
struct FbrGram64ChunkPlan {
    long chb = 0, last_cap = 0, chunks = 0, gram_rounds = 0, prod_rounds = 0;
};
static inline FbrGram64ChunkPlan fbr_gram64_chunk_plan(long nblocks, long cap, long num_cus, long pgrid_max, int rule)
{
    auto plan = [&](long chb, long last_cap) {
        FbrGram64ChunkPlan p;
        p.chb = chb;
        p.last_cap = last_cap;
        const long pb = std::min(chb, pgrid_max);
        for (long left = nblocks; left > 0;) {
            const long nb = left <= last_cap ? left : chb;
            p.chunks++;
            p.gram_rounds += (nb + num_cus - 1) / num_cus;
            p.prod_rounds += (nb + pb - 1) / pb;
            left -= nb;
        }
        return p;
    };
    const long a0 = cap / num_cus;
    FbrGram64ChunkPlan best = plan(a0 * num_cus, a0 * num_cus);
    if (!rule) return best;
    for (long a = a0; a >= 1; a--) {
        const FbrGram64ChunkPlan p = plan(a * num_cus, cap);
        if (p.gram_rounds != best.gram_rounds ? p.gram_rounds < best.gram_rounds
            : p.prod_rounds != best.prod_rounds ? p.prod_rounds < best.prod_rounds
                                                : p.chunks < best.chunks)
            best = p;
    }
    return best;
}

// (the form that takes the tile program too: the pass's tiles are its own, g.tiles)
static inline bool fbr_gram64_build_producer(const FbrHostModel &hm, const FbrGramProgram &, const FbrGram64 &g, FbrGram64Producer &pr)
{
    return fbr_gram64_build_producer(hm, g, pr);
}

// The producer's rhs moments for k rhs columns (k <= FBR_G64_MAXK): per producer workgroup and lane, running sum r * cols + c =
// (w Y_c)^T (w rhs_r), then the upper triangle of (w rhs_i)^T (w rhs_j) row by row (k = 2: 00, 01, 11).  k = 1: [cols + 1].
#define FBR_G64_MAXK 2
#include "fbr_mom_lanes.h"  // fbr_gram64_mom_lane, fbr_mom_lanes_sum: the sum of a moment over the lanes of a wave
FBR_HD int fbr_gram64_mom_count(int cols, int k) { return k * cols + k * (k + 1) / 2; }
// the entry (row, col), row <= col, of the (cols + k)^2 Gram that running sum idx belongs to (its mirror image too when row != col)
FBR_HD void fbr_gram64_mom_target(int cols, int k, int idx, int *row, int *col)
{
    if (idx < k * cols) {
        *row = idx % cols;
        *col = cols + idx / cols;
        return;
    }
    int e = idx - k * cols, i = 0;
    while (e >= k - i) e -= k - i, i++;
    *row = cols + i;
    *col = cols + i + e;
}

// What the lanes of a producer wave add a link's moments to, [nparts][L][64]: lane fbr_gram64_mom_lane(p, r) of (part, link) holds column
// lcol[p] of that part and link | r << 24 (r: the rhs column), lane fbr_gram64_mom_fric_lane(pf, r) the friction column pf of the link's
// joint; every other lane, and the lane of a column the part does not write, -1.  One coalesced load per link gives a lane its running sum.
#define FBR_G64_LANECOL_RHS 24
static inline std::vector<int> fbr_gram64_lane_columns(const FbrGram64Producer &pr, int L)
{
    std::vector<int> t((size_t)pr.nparts * L * 64, -1);
    for (int pq = 0; pq < pr.nparts; pq++)
        for (int l = 0; l < L; l++)
            for (int r = 0; r < FBR_G64_MAXK; r++) {
                int *row = &t[((size_t)pq * L + l) * 64];
                for (int p = 0; p < 10; p++) {
                    const int c = pr.lcol[((size_t)pq * L + l) * 10 + p];
                    if (c >= 0) row[fbr_gram64_mom_lane(p, r)] = c | r << FBR_G64_LANECOL_RHS;
                }
                for (int pf = 0; pf < FBR_G64_FRIC; pf++) {
                    const int c = pr.lcol[(size_t)pr.nparts * 10 * L + ((size_t)pq * L + l) * FBR_G64_FRIC + pf];
                    if (c >= 0) row[fbr_gram64_mom_fric_lane(pf, r)] = c | r << FBR_G64_LANECOL_RHS;
                }
            }
    return t;
}

#if defined(__HIPCC__) && defined(FBR_KERNELS_GRAM)
// The exchanges of fbr_mom_lanes_sum on the device: register moves only (v_permlane32_swap / v_permlane16_swap of gfx950 for the halves
// and the rows, DPP moves inside a row) -- nothing through the LDS, nothing on lgkmcnt.  Every lane of the wave must be running.
struct FbrMomLanesDev {
    int lane;
    template <int CTRL>
    static __device__ __forceinline__ double dpp(double v)
    {
        const long b = __builtin_bit_cast(long, v);
        const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xf, 0xf, true), hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, true);
        return __builtin_bit_cast(double, ((long)(unsigned)hi << 32) | (long)(unsigned)lo);
    }
    static __device__ __forceinline__ void put(double &a, double &b, unsigned l0, unsigned l1, unsigned h0, unsigned h1)
    {
        a = __builtin_bit_cast(double, ((long)h0 << 32) | (long)l0);
        b = __builtin_bit_cast(double, ((long)h1 << 32) | (long)l1);
    }
    __device__ __forceinline__ void swap32(double &a, double &b) const
    {
        const long x = __builtin_bit_cast(long, a), y = __builtin_bit_cast(long, b);
        const auto l = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)y, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap((unsigned)(x >> 32), (unsigned)(y >> 32), false, false);
        put(a, b, l[0], l[1], h[0], h[1]);
    }
    __device__ __forceinline__ void swap16(double &a, double &b) const
    {
        const long x = __builtin_bit_cast(long, a), y = __builtin_bit_cast(long, b);
        const auto l = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)y, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap((unsigned)(x >> 32), (unsigned)(y >> 32), false, false);
        put(a, b, l[0], l[1], h[0], h[1]);
    }
    __device__ __forceinline__ double get8(double a) const { return dpp<0x128>(a); }  // row_ror:8
    __device__ __forceinline__ double get7(double a) const { return dpp<0x141>(a); }  // row_half_mirror
    __device__ __forceinline__ double get2(double a) const { return dpp<0x4E>(a); }   // quad_perm:[2,3,0,1]
    __device__ __forceinline__ double get1(double a) const { return dpp<0xB1>(a); }   // quad_perm:[1,0,3,2]
    __device__ __forceinline__ double live0(bool live, double a) const { return live ? a : 0.0; }
    __device__ __forceinline__ double bit8(double a, double b) const { return (lane & 8) ? b : a; }
    __device__ __forceinline__ double zero() const { return 0.0; }
};

struct DevGram64 {
    int NT, nlev, maxact, npieces, nstage;  // NT: main + force tiles
    long blk_doubles;
    const int *slab, *lev_begin, *pieces, *wmeta, *stage_lev;
    const int *runs;  // [WPB][nlev] (FbrGram64::runs) or null
};

// ------------------------------------------------------------------------------------------------
// Producer: the lane writer of fbr_kinid.h with the image addressing of this pass.  Destination word of a (column, row): address of the
// slab position of column slot c, sample 0 (256-byte aligned) | the slot's swizzle in its low byte; sample slot s of block b goes to
// + b * blk_doubles + (s >> 5) * 512 + ((s & 31) ^ x).  ALL 64 lanes of the last block of a group run: the lanes behind its last sample walk the tree on that
// sample (the wave-wide sums below exchange registers between lanes, which must be defined) and write its values to their own positions, which
// fbr_gram64_tail_zero_kernel clears AFTER this kernel (the Gram kernel runs whole blocks).  mom (k >= 1; KR = max(k, 1) rhs columns, row-major [S rows][k]):
// [workgroup][fbr_gram64_mom_count] running sums of (w Y)^T (w rhs_r) per column and of (w rhs_i)^T (w rhs_j).  A link's products are summed over the live lanes
// of the wave in registers (fbr_mom_lanes_sum: a fixed order), lane fbr_gram64_mom_lane(p, r) ends up with the sum of parameter p for rhs column r, and ONE no-return atomic per
// (part, link) adds them, each lane to the running sum of its own column; one wave adds to an address, in block order.  The KR = 1 instances serve
// k = 0 and k = 1.
// ------------------------------------------------------------------------------------------------
template <int MAXD, bool HASW, int KR = 1>
__global__ __launch_bounds__(64 * FBR_KINWRITE_PARTS, MAXD <= 10 ? 2 : 1) void fbr_kinimg_kernel(DevModel m, DevKinId p, DevKinWrite wr, long S, long blk_doubles,
                                                                              const double *__restrict__ q, const double *__restrict__ dq,
                                                                              const double *__restrict__ ddq, const double *__restrict__ bv,
                                                                              const double *__restrict__ ba, const double *__restrict__ rpy,
                                                                              const double *__restrict__ rhs, const double *__restrict__ wts,
                                                                              double *__restrict__ scratch, double *__restrict__ mom,
                                                                              const double *__restrict__ sign)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x & 63, part = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nth = blockDim.x, tid = threadIdx.x;
    const int n = m.n, ldn = p.ldn, ldw = m.rows | 1, rows = m.rows;
    double *sq = smem, *sdq = sq + 64 * ldn, *sddq = sdq + 64 * ldn, *sw = sddq + 64 * ldn;  // sw [64][ldw] row weights (has_w)
    double *st = sw + (HASW ? 64 * ldw : 0);                                             // st [KR][64][ldw] w^2 rhs_r (k >= 1)
    double *scr = scratch + ((long)blockIdx.x * wr.nparts + part) * p.nslots * FBR_LINK_REC * 64 + lane;
    double *mo = mom ? mom + (long)blockIdx.x * (KR * wr.cols + KR * (KR + 1) / 2) : nullptr;  // [fbr_gram64_mom_count(cols, KR)]
    const bool domom = KR > 1 || wr.k != 0;
    const FbrMomLanesDev mx{lane};
    // sample groups (fbr_gram_grouped): every group starts a block -- block b = (group b / bpg, block b % bpg of the group)
    const long Sg = wr.group_samples > 0 ? wr.group_samples : S, bpg = (Sg + 63) >> 6;
    const long nblk = (S / Sg) * bpg;
    const fbr_clong_ptr cdst = (fbr_clong_ptr)(unsigned long)wr.dst;
    // what this lane adds the moments of (part, link 0) to (fbr_gram64_lane_columns); a global load: vmcnt only
    const __attribute__((address_space(1))) int *glcol = (const __attribute__((address_space(1))) int *)(unsigned long)wr.lanecol + (long)part * m.L * 64 + lane;
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long grp = blk / bpg, lb = blk - grp * bpg;
        const long base = grp * Sg + (lb << 6);
        const int valid = (int)min(64L, Sg - (lb << 6));
        __syncthreads();
        {
            const long off = base * n;
            const int cnt = valid * n;
            int sr = tid / n, dc = tid - sr * n;
            const int ds = nth / n, dd = nth - ds * n;
            for (int i = tid; i < cnt; i += nth) {
                const double a = q[off + i], b = dq[off + i], c = ddq[off + i];
                sq[sr * ldn + dc] = a;
                sdq[sr * ldn + dc] = b;
                sddq[sr * ldn + dc] = c;
                sr += ds;
                dc += dd;
                if (dc >= n) {
                    dc -= n;
                    sr++;
                }
            }
            if (HASW || wr.k) {
                const int cw = valid * rows;
                int wr_ = tid / rows, wc = tid - wr_ * rows;
                const int es = nth / rows, ed = nth - es * rows;
                for (int i = tid; i < cw; i += nth) {
                    const double wv = HASW ? wts[base * rows + i] : 1.0;
                    if (HASW) sw[wr_ * ldw + wc] = wv;
                    if constexpr (KR == 1) {
                        if (wr.k) st[wr_ * ldw + wc] = wv * wv * rhs[base * rows + i];
                    } else {
#pragma unroll
                        for (int r = 0; r < KR; r++) st[r * 64 * ldw + wr_ * ldw + wc] = wv * wv * rhs[(base * rows + i) * KR + r];
                    }
                    wr_ += es;
                    wc += ed;
                    if (wc >= rows) {
                        wc -= rows;
                        wr_++;
                    }
                }
            }
        }
        __syncthreads();
        const int ls = min(lane, valid - 1);
        const long s = base + ls;
        const bool live = lane < valid;
        const double *mysq = sq + ls * ldn, *mysdq = sdq + ls * ldn, *mysddq = sddq + ls * ldn, *myw = sw + ls * ldw, *myt = st + ls * ldw;
        const long slot_off = blk * blk_doubles + (long)(lane >> 5) * 512;
        const int s31 = lane & 31;
        auto state = [&](int d, double &a, double &b, double &c) {
            a = mysq[d];
            b = mysdq[d];
            c = mysddq[d];
        };
        auto basest = [&](double *v6, double *a6, double *e3) {
            for (int i = 0; i < 6; i++) {
                v6[i] = bv[s * 6 + i];
                a6[i] = ba[s * 6 + i];
            }
            for (int i = 0; i < 3; i++) e3[i] = rpy[s * 3 + i];
        };
        auto save = [&](int b, int i, double v) { scr[(b * FBR_LINK_REC + i) * 64] = v; };
        auto load = [&](int b, int i) { return scr[(b * FBR_LINK_REC + i) * 64]; };
        auto consts = [&](int l, double *rR, double *rp, double *ax) {  // (l is wave-uniform: scalar loads through the constant address space)
            const fbr_cdouble_ptr cR = (fbr_cdouble_ptr)(unsigned long)m.restR, cp = (fbr_cdouble_ptr)(unsigned long)m.restp,
                                  ca = (fbr_cdouble_ptr)(unsigned long)m.axis;
            for (int i = 0; i < 9; i++) rR[i] = cR[9 * l + i];
            for (int i = 0; i < 3; i++) {
                rp[i] = cp[3 * l + i];
                ax[i] = ca[3 * l + i];
            }
        };
        // byte offset of this lane's sample inside a (tile row, column) run, before the column's swizzle: block, half, sample
        const unsigned vlane = (unsigned)(((unsigned long)slot_off + (unsigned long)s31) << 3);
        auto link = [&](int l, int depth, const double *rec, const double (*Sst)[6], const int *lvd, double *F) {
            (void)F;
            if (wr.base_only) depth = 0;  // (row weights switch every joint row off: identifier.py:629-636 -- only the base-wrench rows are produced)
            // (option gram_lane_skip_unowned) a link none of whose columns this part writes -- an ancestor walked for its kinematics: nothing
            // to load, wait for, form or add.  The flag is the wave's: one scalar load.
            if (wr.none && ((fbr_cint_ptr)(unsigned long)wr.none)[(long)part * m.L + l]) return;
            // Every vector load of the step (branch records, states) is waited for HERE, once: the stores below share the loads' counter, and
            // behind the branches of the column code the compiler cannot tell how many of them sit in front of a load it still expects --
            // it would wait for counter 0, i.e. for the store before, at every store (measured: 7.4 -> 5.4 ms per 1 M WALK-MAN samples).
            // (the running sum this lane adds to at the end of the link, or -1: one vector load, in front of the wait, which it shares)
            int mycol = -1;
            if (domom) mycol = glcol[l * 64];
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt / lgkmcnt untouched
            // what this lane adds: the groups' sums land in it by lane pattern (fbr_gram64_mom_lane: parameters 0 .. 3 in lanes 0 mod 16, 4 .. 9 in lanes 1 mod
            // 8, rhs column 1 six lanes further on; the classes of absent columns hold exact zeros), the lanes that matter are those with a column
            double macc = 0.0;
            // the products of parameters P0 .. P0 + NQ - 1 (v: [NQ]) summed over the wave, at their places in the group of NG parameters that starts at G0
            auto mom_sum = [&](auto g0c, auto ngc, auto p0c, auto nqc, const double *v, int r) {
                constexpr int G0 = decltype(g0c)::value, NG = decltype(ngc)::value, P0 = decltype(p0c)::value, NQ = decltype(nqc)::value;
                double u[NG];
#pragma unroll
                for (int i = 0; i < NG; i++) u[i] = (G0 + i >= P0 && G0 + i < P0 + NQ) ? v[G0 + i - P0] : 0.0;
                const double sum = fbr_mom_lanes_sum<NG>(u, live, mx);
                if (G0 == 0 ? (lane & 15) == 6 * r : (lane & 7) == 1 + 6 * r) macc += sum;
            };
            long d10[10], dF[4];
#pragma unroll
            for (int pp = 0; pp < 10; pp++) d10[pp] = cdst[((long)part * m.L + l) * FBR_G64_WORDS + pp];
#pragma unroll
            for (int pp = 0; pp < 4; pp++) dF[pp] = cdst[((long)part * m.L + l) * FBR_G64_WORDS + 10 + pp];  // force-tile words (rows 0 .. flev-1)
            // the rhs side of the moments: sum_r v_r t_r over the rows of one column = w6 . (t_base + sum_j S_j t_j), t = w^2 rhs_r: one
            // six-vector per rhs column.  F = w^2 rhs_r's, from this lane's staged row at LDS offset ro
            auto ft_of = [&](int ro, double *F) {
#pragma unroll
                for (int i = 0; i < 6; i++)
                    if (i < m.fb) F[i] = myt[ro + i];
#pragma unroll
                for (int j = 0; j < MAXD; j++)
                    if (j < depth) {
                        const double tj = myt[ro + m.fb + lvd[j]];
#pragma unroll
                        for (int i = 0; i < 6; i++) F[i] += Sst[j][i] * tj;
                    }
            };
            double Ft[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if constexpr (KR == 1) {
                if (wr.k) {
#pragma unroll
                    for (int i = 0; i < 6; i++)
                        if (i < m.fb) Ft[i] = myt[i];
#pragma unroll
                    for (int j = 0; j < MAXD; j++)
                        if (j < depth) {
                            const double tj = myt[m.fb + lvd[j]];
#pragma unroll
                            for (int i = 0; i < 6; i++) Ft[i] += Sst[j][i] * tj;
                        }
                }
            }
            // KR > 1: the instances sit at their register bound with ONE such vector live (two waves per SIMD at 256 registers up to depth
            // 10), so every column group rebuilds the vector of each rhs column in front of its products instead of keeping KR of them for
            // the whole link.  The offset is made opaque: the compiler would otherwise hoist the KR vectors out of the groups again.
            auto ft_group = [&](int r, double *F) {
                int ro = r * 64 * ldw;
                asm volatile("" : "+v"(ro));
#pragma unroll
                for (int i = 0; i < 6; i++) F[i] = 0.0;
                ft_of(ro, F);
            };
            // One value to (column q of the group, level lv).  Scalar base (the column's word, 8192 bytes per level) + this lane's 32-bit
            // offset with the column's swizzle; a column the part does not write (word 0) skips the store only -- the products of a level
            // are computed for the whole group first, branch-free, so that their dependent chains overlap (the compiler keeps them outside
            // the store branches).  A link with no written column at all has returned before it got here (wr.none).
            using std::integral_constant;
            auto store = [&](long d0, int lv, double v) {
                if (d0 == 0) return;
                const unsigned vo = vlane ^ ((unsigned)(d0 & 0xff) << 3);
                __builtin_nontemporal_store(v, (fbr_gdouble_ptr)((fbr_gchar_ptr)(d0 & ~0xffL) + (long)lv * 8192 + vo));
            };
            // mass and first moments: full wrenches, NQ columns at a time
            auto full_group = [&](auto q0c, auto nqc) {
                constexpr int Q0 = decltype(q0c)::value, NQ = decltype(nqc)::value;
                double wA[NQ][6];
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) fbr_unit_wrench(rec, Q0 + qq, wA[qq]);
#pragma unroll
                for (int i = 0; i < 6; i++)
                    if (i < m.fb) {
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) store(i < wr.flev ? dF[Q0 + qq] : d10[Q0 + qq], i, HASW ? wA[qq][i] * myw[i] : wA[qq][i]);
                    }
#pragma unroll
                for (int j = 0; j < MAXD; j++)
                    if (j < depth) {
                        double v[NQ];
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) v[qq] = fbr_dot6(Sst[j], wA[qq]);
                        const double wj = HASW ? myw[m.fb + lvd[j]] : 1.0;
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) store(d10[Q0 + qq], m.fb + j, HASW ? v[qq] * wj : v[qq]);
                    }
                long any = 0;  // (a group none of whose columns the part writes has no sums)
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) any |= d10[Q0 + qq];
                if (!domom || any == 0) return;
                double v[NQ];
                if constexpr (KR == 1) {
#pragma unroll
                    for (int qq = 0; qq < NQ; qq++) v[qq] = fbr_dot6(Ft, wA[qq]);
                    mom_sum(integral_constant<int, 0>{}, integral_constant<int, 4>{}, q0c, nqc, v, 0);
                } else {
#pragma unroll
                    for (int r = 0; r < KR; r++) {
                        double F[6];
                        ft_group(r, F);
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) v[qq] = fbr_dot6(F, wA[qq]);
                        mom_sum(integral_constant<int, 0>{}, integral_constant<int, 4>{}, q0c, nqc, v, r);
                    }
                }
            };
            // inertia entries: pure moments -- the force rows of the base wrench are structural zeros of the image (never written), the joint
            // rows need the moment half of S only
            auto moment_group = [&](auto q0c, auto nqc) {
                constexpr int Q0 = decltype(q0c)::value, NQ = decltype(nqc)::value;
                double nB[NQ][3];
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) fbr_unit_moment3(rec, 4 + Q0 + qq, nB[qq]);
#pragma unroll
                for (int i = 3; i < 6; i++)
                    if (i < m.fb) {
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) store(d10[4 + Q0 + qq], i, HASW ? nB[qq][i - 3] * myw[i] : nB[qq][i - 3]);
                    }
#pragma unroll
                for (int j = 0; j < MAXD; j++)
                    if (j < depth) {
                        double v[NQ];
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) v[qq] = Sst[j][3] * nB[qq][0] + Sst[j][4] * nB[qq][1] + Sst[j][5] * nB[qq][2];
                        const double wj = HASW ? myw[m.fb + lvd[j]] : 1.0;
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) store(d10[4 + Q0 + qq], m.fb + j, HASW ? v[qq] * wj : v[qq]);
                    }
                long any = 0;
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) any |= d10[4 + Q0 + qq];
                if (!domom || any == 0) return;
                double v[NQ];
                if constexpr (KR == 1) {
#pragma unroll
                    for (int qq = 0; qq < NQ; qq++) v[qq] = Ft[3] * nB[qq][0] + Ft[4] * nB[qq][1] + Ft[5] * nB[qq][2];
                    mom_sum(integral_constant<int, 4>{}, integral_constant<int, 6>{}, integral_constant<int, 4 + Q0>{}, nqc, v, 0);
                } else {
#pragma unroll
                    for (int r = 0; r < KR; r++) {
                        double F[6];
                        ft_group(r, F);
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) v[qq] = F[3] * nB[qq][0] + F[4] * nB[qq][1] + F[5] * nB[qq][2];
                        mom_sum(integral_constant<int, 4>{}, integral_constant<int, 6>{}, integral_constant<int, 4 + Q0>{}, nqc, v, r);
                    }
                }
            };
            if constexpr (MAXD > 8 && MAXD <= 10) {  // (the instance that has to fit 256 registers for two waves per SIMD: smaller groups)
                full_group(integral_constant<int, 0>{}, integral_constant<int, 2>{});
                full_group(integral_constant<int, 2>{}, integral_constant<int, 2>{});
                moment_group(integral_constant<int, 0>{}, integral_constant<int, 3>{});
                moment_group(integral_constant<int, 3>{}, integral_constant<int, 3>{});
            } else {
                full_group(integral_constant<int, 0>{}, integral_constant<int, 4>{});
                moment_group(integral_constant<int, 0>{}, integral_constant<int, 6>{});
            }
            // friction columns of the link's own joint: one value each, on the row of that joint (the last level of the link's path)
            const int nfr = wr.cols > wr.ninert ? (wr.cols - wr.ninert) / n : 0;
            const int dj = nfr ? m.dof[l] : -1;
            if (dj >= 0 && depth > 0) {
                const fbr_cint_ptr cfr = (fbr_cint_ptr)(unsigned long)(wr.lcol10 + (long)wr.nparts * 10 * m.L + ((long)part * m.L + l) * FBR_G64_FRIC);
#pragma unroll
                for (int pf = 0; pf < FBR_G64_FRIC; pf++)
                    if (pf < nfr) {
                        const long dfw = cdst[((long)part * m.L + l) * FBR_G64_WORDS + 14 + pf];
                        if (dfw == 0) continue;
                        const int c = cfr[pf];
                        const double fv = fbr_friction_value(m.coldesc[c].z, mysdq[dj], sign ? sign[s * n + dj] : 0.0, m.stribeck);
                        store(dfw, m.fb + depth - 1, HASW ? fv * myw[m.fb + dj] : fv);
                        if (!domom) continue;
#pragma unroll
                        for (int r = 0; r < KR; r++) {  // (one value: every lane gets the sum, lane fbr_gram64_mom_fric_lane(pf, r) keeps it)
                            const double v = fv * myt[r * 64 * ldw + m.fb + dj], sum = fbr_mom_lanes_sum<1>(&v, live, mx);
                            if (lane == fbr_gram64_mom_fric_lane(pf, r)) macc = sum;
                        }
                    }
            }
            // the link's sums: lane fbr_gram64_mom_lane(p, r) adds parameter p's for rhs column r, to the running sum of its column (-1: the part does not
            // write it) -- one atomic per link
            if (domom && mycol >= 0 && (KR > 1 || mycol < (1 << FBR_G64_LANECOL_RHS)))
                unsafeAtomicAdd(mo + (mycol >> FBR_G64_LANECOL_RHS) * wr.cols + (mycol & ((1 << FBR_G64_LANECOL_RHS) - 1)), macc);
        };
        auto emit = [&](int, double) {};
        // (all lanes: the ones behind the last sample of the last block repeat that sample, see above)
        {
            fbr_kinid_lane<MAXD, false>(wr.part_nsteps[part], p.maxlvl, p.steps + wr.part_step0[part] * FBR_KINID_STEP, p.endflush, m.floating, m.g, m.fb,
                                        state, basest, save, load, link, emit, consts);
            if constexpr (KR == 1) {
                if (wr.k && part == wr.nparts - 1) {  // (w tau)^T (w tau)
                    double tt = 0.0;
                    for (int r = 0; r < rows; r++) {
                        const double wv = HASW ? myw[r] : 1.0, tv = rhs[s * rows + r] * wv;
                        tt += tv * tv;
                    }
                    const double sum = fbr_mom_lanes_sum<1>(&tt, live, mx);
                    if (lane == 0) unsafeAtomicAdd(mo + wr.cols, sum);
                }
            } else if (part == wr.nparts - 1) {  // (w rhs_i)^T (w rhs_j), i <= j, row by row
                double tt[KR * (KR + 1) / 2];
#pragma unroll
                for (int e = 0; e < KR * (KR + 1) / 2; e++) tt[e] = 0.0;
                for (int r = 0; r < rows; r++) {
                    const double wv = HASW ? myw[r] : 1.0;
                    double tv[KR];
#pragma unroll
                    for (int i = 0; i < KR; i++) tv[i] = rhs[(s * rows + r) * KR + i] * wv;
#pragma unroll
                    for (int i = 0, e = 0; i < KR; i++)
#pragma unroll
                        for (int j = i; j < KR; j++, e++) tt[e] += tv[i] * tv[j];
                }
                double mine = 0.0;  // (entry e in lane e, one atomic for the corner)
#pragma unroll
                for (int e = 0; e < KR * (KR + 1) / 2; e++) {
                    const double sum = fbr_mom_lanes_sum<1>(&tt[e], live, mx);
                    if (lane == e) mine = sum;
                }
                if (lane < KR * (KR + 1) / 2) unsafeAtomicAdd(mo + (long)KR * wr.cols + lane, mine);
            }
        }
    }
}

// The positions of sample slots valid .. 63 of the LAST block of every group (blockIdx.y; bpg blocks per group): groups whose sample count is
// no multiple of 64 end in a block the producer fills partly, and an image buffer is reused from call to call.
__global__ __launch_bounds__(256) void fbr_gram64_tail_zero_kernel(double *__restrict__ img, long blk_doubles, long bpg, int ntr, int valid)
{
    double *blk = img + ((long)blockIdx.y * bpg + bpg - 1) * blk_doubles;
    const int per = 16 * (64 - valid);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)ntr * per; e += (long)gridDim.x * blockDim.x) {
        const int tr = (int)(e / per), r = (int)(e - (long)tr * per), c = r / (64 - valid), sl = valid + r % (64 - valid);
        blk[(long)tr * 1024 + (sl >> 5) * 512 + c * 32 + ((sl & 31) ^ FBR_G64_SWZ(c))] = 0.0;
    }
}

// rhs moments of a call -> G (k rhs columns): one wave per running sum (fbr_gram64_mom_count of them, four to a workgroup) adds up that
// sum's copies of the producer's nwg workgroups in a fixed order; where it goes in G: fbr_gram64_mom_target
__global__ __launch_bounds__(256) void fbr_gram64_mom_reduce_kernel(int P, int k, int nwg, const double *__restrict__ mom, double *__restrict__ G)
{
    __shared__ double part[4][64];
    const int w = threadIdx.x >> 6, t = threadIdx.x & 63, nm = fbr_gram64_mom_count(P, k), c = blockIdx.x * 4 + w;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;  // (independent running sums: the loads are far apart)
    if (c < nm) {
        int i = t;
        for (; i + 192 < nwg; i += 256) {
            s0 += mom[(long)i * nm + c];
            s1 += mom[(long)(i + 64) * nm + c];
            s2 += mom[(long)(i + 128) * nm + c];
            s3 += mom[(long)(i + 192) * nm + c];
        }
        for (; i < nwg; i += 64) s0 += mom[(long)i * nm + c];
    }
    part[w][t] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if (t < o) part[w][t] += part[w][t + o];
        __syncthreads();
    }
    if (t || c >= nm) return;
    const int Pa = P + k;
    int row, col;
    fbr_gram64_mom_target(P, k, c, &row, &col);
    G[(long)row * Pa + col] += part[w][0];
    if (row != col) G[(long)col * Pa + row] += part[w][0];
}

// ------------------------------------------------------------------------------------------------
// Consumer.  One workgroup (8 waves) per CU walks blocks blockIdx.x, + gridDim.x, ...; stage = (block, half, level).  partial:
// [workgroup][wave][slot][4][64] (the layout fbr_gram_reduce_kernel sums); carry: start from it.
// ------------------------------------------------------------------------------------------------
template <int NPW, int WPB, bool RUNS = false>
__global__ __launch_bounds__(WPB * 64, (NPW <= 10) ? 4 : 2) void fbr_gram64_kernel(DevGram64 g, long nblk, const double *__restrict__ img,
                                                                                  double *__restrict__ partial, int carry)
{
    constexpr int MW = 3 * NPW;
    static_assert(MW <= 64, "a wave's slot table is fetched with one load");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int bufd = g.maxact * 512;
    double *buf0 = smem, *buf1 = smem + bufd;
    int *slab = (int *)(smem + 2 * bufd);      // [nlev][NT]
    int *levb = slab + g.nlev * g.NT;          // [nlev + 1]
    int *pcs = levb + g.nlev + 1;              // [npieces][2]
    int *wm = pcs + 2 * g.npieces;             // [8][NPW][3]
    int *rn = wm + WPB * MW;                   // [8][nlev] runs (when the table is there)
    static_assert(!RUNS || NPW > 10, "the 128-register shapes walk every slot");
    int *stl = rn + (RUNS ? WPB * g.nlev : 0);  // [nstage + 1]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < g.nlev * g.NT; i += WPB * 64) slab[i] = g.slab[i] * 512;  // (in doubles)
    for (int i = tid; i <= g.nlev; i += WPB * 64) levb[i] = g.lev_begin[i];
    for (int i = tid; i < 2 * g.npieces; i += WPB * 64) pcs[i] = g.pieces[i];
    for (int i = tid; i < WPB * MW; i += WPB * 64) wm[i] = g.wmeta[i];
    if (RUNS)
        for (int i = tid; i < WPB * g.nlev; i += WPB * 64) rn[i] = g.runs[i];
    for (int i = tid; i <= g.nstage; i += WPB * 64) stl[i] = g.stage_lev[i];
    fbr_d4 acc[NPW];
    img += (long)blockIdx.y * nblk * g.blk_doubles;  // blockIdx.y: sample group (nblk blocks each, fbr_gram_grouped)
    // partial sums in the order of fbr_gram_reduce_kernel (8 rows per workgroup): wave w is row w & 7, slots (w >> 3) NPW ...
    double *pp = partial + (((((long)blockIdx.y * gridDim.x + blockIdx.x) * 8 + (wave & 7)) * (WPB / 8) + (wave >> 3)) * NPW) * 256;
    if (carry) {
#pragma unroll
        for (int q = 0; q < NPW; q++) acc[q] = (fbr_d4){pp[q * 256 + lane], pp[q * 256 + 64 + lane], pp[q * 256 + 128 + lane], pp[q * 256 + 192 + lane]};
    } else {
#pragma unroll
        for (int q = 0; q < NPW; q++) acc[q] = (fbr_d4){0.0, 0.0, 0.0, 0.0};
    }
    __syncthreads();
    const int nmine = (int)((nblk - blockIdx.x + gridDim.x - 1) / gridDim.x);  // blocks of this workgroup
    const long nst = (long)(nmine > 0 ? nmine : 0) * 2 * g.nstage;
    // per-stage constants in registers (lane s: stage s; lane nstage: the end): first level and first DMA piece -- read with a lane select
    // instead of chained LDS look-ups in front of every stage
    const int svl = stl[lane <= g.nstage ? lane : 0], svp = levb[svl];
    // LDS-DMA of step (block-half bh, stage sg) into buffer par: wave w issues pieces w, w + WPB, ... of the stage's levels
    auto dma = [&](int sg, long bh, int par) {
        const long blk = (long)blockIdx.x + (bh >> 1) * gridDim.x;
        const double *src = img + blk * g.blk_doubles + (bh & 1) * 512 + 2 * lane;
        double *buf = par ? buf1 : buf0;
        // (the wave's pieces i0, i0 + WPB, ... of the stage: their table entries are fetched by the lanes in parallel -- one LDS round trip
        // instead of one per piece in front of every stage's first MFMA)
        const int i0 = __builtin_amdgcn_readlane(svp, sg) + wave, i1 = __builtin_amdgcn_readlane(svp, sg + 1);
        const int mine = i0 < i1 ? (i1 - i0 + WPB - 1) / WPB : 0;
        const int il = i0 + (lane < mine ? lane : 0) * WPB;
        const int gxv = mine > 0 ? pcs[2 * il] : 0, lxv = mine > 0 ? pcs[2 * il + 1] : 0;
        for (int j = 0; j < mine; j++) {
            const int gx = __builtin_amdgcn_readlane(gxv, j), lx = __builtin_amdgcn_readlane(lxv, j);
            __builtin_amdgcn_global_load_lds((fbr_glb_ptr)(src + gx), (fbr_lds_ptr)(buf + lx), 16, 0, 0);
        }
    };
    if (nst > 0) dma(0, 0, 0);
    const int li = lane & 15, kk = lane >> 4;
    const int lofs = li * 32, sx = FBR_G64_SWZ(li);
    const int mv = wm[wave * MW + (lane < MW ? lane : 0)];  // this wave's slots: (tile I, tile J, first level | end level << 8)
    const int idxv = (lane < MW && (lane % 3) != 2 && mv >= 0) ? mv : 0;  // the tile this lane looks up per level (lanes 3q, 3q + 1)
    // this lane's operand position inside a slab (doubles) at k-step ks: column li, sample (4 ks + kk) ^ sx = p0 ^ (4 ks)
    const int p0c = lofs | (sx ^ kk);
    // runs: one LDS read per level gives the slab offsets of all slots (lanes 3q, 3q + 1) and, in lane 63, the level's run of active slots
    static_assert(!RUNS || MW < 63, "lane 63 holds the run");
    const int *lk = lane == 63 ? rn + wave * g.nlev : slab + idxv;
    const int lks = lane == 63 ? 1 : g.NT;
    // The levels of a stage with runs: the slots qa .. qb-1 of a level as one software pipeline.  Slot q's operands sit in set q & 1; the
    // operand reads of slot q + 1 (B, then A -- or a copy of slot q's A when slot q + 1 has the same tile I) go out between slot q's MFMAs,
    // so that slot q + 1 finds them landed.  The reads are inline asm (one statement per slot, its choice of B only / B + A / B + copy
    // inside it; one more for the first slot's own reads): the compiler neither counts them nor sees a join behind which it would wait for every read, so a slot waits for its own
    // reads only.  The slots outside the run are branched over.  Every accumulator receives the same MFMAs in the same order as in the walk
    // below.
    const unsigned rlm = [&] {  // bit q: slot q holds another tile I than slot q - 1 (its A operand is read, not copied)
        unsigned m = 0;
#pragma unroll
        for (int q = 1; q < NPW; q++) m |= (unsigned)(__builtin_amdgcn_readlane(mv, 3 * q) != __builtin_amdgcn_readlane(mv, 3 * q - 3)) << q;
        return (unsigned)__builtin_amdgcn_readfirstlane((int)m);
    }();
    int ko[8];  // this lane's operand byte offsets inside a slab, k-steps 0 .. 7
#pragma unroll
    for (int ks = 0; ks < 8; ks++) ko[ks] = (p0c ^ (4 * ks)) * 8;
    double X[2][8], Y[2][8];  // operand sets A, B of the even / odd slots
#pragma unroll
    for (int ks = 0; ks < 8; ks++) X[0][ks] = X[1][ks] = Y[0][ks] = Y[1][ks] = 0.0;
    auto run_stage = [&](const double *buf, int lv0, int lv1) {
        const unsigned bufb = (unsigned)(unsigned long)(fbr_lds_ptr)buf;
        int offv = lk[lv0 * lks];
        for (int lv = lv0; lv < lv1; lv++) {
            const int cur = offv;
            offv = lk[(lv + 1 < g.nlev ? lv + 1 : lv) * lks];  // the next level's offsets, in flight during this level
            const int run = __builtin_amdgcn_readlane(cur, 63), qa = run & 0xff, qb = run >> 8;
#define G64_RD(D, S, K, T) "v_add_u32 %[" T "], %[" S "], %[o" #K "]\n\tds_read_b64 %[" D #K "], %[" T "]\n\t"
#define G64_MF(K) "v_mfma_f64_16x16x4_f64 %[acc], %[xa" #K "], %[xb" #K "], %[acc]\n\t"
#define G64_MV(K) "v_mov_b64 %[ya" #K "], %[xa" #K "]\n\t"
#pragma unroll
            for (int q = 0; q < NPW; q++) {
                if (q < qa || q >= qb) continue;
                const int P = q & 1, N = P ^ 1;
                int t0, t1;
                if (q == qa) {  // the first slot of the run reads its own operands
                    const unsigned sa = bufb + (__builtin_amdgcn_readlane(cur, 3 * q) << 3), sb = bufb + (__builtin_amdgcn_readlane(cur, 3 * q + 1) << 3);
                    asm volatile(G64_RD("xa", "sa", 0, "t0") G64_RD("xa", "sa", 1, "t1") G64_RD("xa", "sa", 2, "t0") G64_RD("xa", "sa", 3, "t1")
                                 G64_RD("xa", "sa", 4, "t0") G64_RD("xa", "sa", 5, "t1") G64_RD("xa", "sa", 6, "t0") G64_RD("xa", "sa", 7, "t1")
                                 G64_RD("xb", "sb", 0, "t0") G64_RD("xb", "sb", 1, "t1") G64_RD("xb", "sb", 2, "t0") G64_RD("xb", "sb", 3, "t1")
                                 G64_RD("xb", "sb", 4, "t0") G64_RD("xb", "sb", 5, "t1") G64_RD("xb", "sb", 6, "t0") G64_RD("xb", "sb", 7, "t1")
                                 : [t0] "=&v"(t0), [t1] "=&v"(t1),
                                   [xa0] "+v"(X[P][0]), [xa1] "+v"(X[P][1]), [xa2] "+v"(X[P][2]), [xa3] "+v"(X[P][3]),
                                   [xa4] "+v"(X[P][4]), [xa5] "+v"(X[P][5]), [xa6] "+v"(X[P][6]), [xa7] "+v"(X[P][7]),
                                   [xb0] "+v"(Y[P][0]), [xb1] "+v"(Y[P][1]), [xb2] "+v"(Y[P][2]), [xb3] "+v"(Y[P][3]),
                                   [xb4] "+v"(Y[P][4]), [xb5] "+v"(Y[P][5]), [xb6] "+v"(Y[P][6]), [xb7] "+v"(Y[P][7])
                                 : [sa] "s"(sa), [sb] "s"(sb),
                                   [o0] "v"(ko[0]), [o1] "v"(ko[1]), [o2] "v"(ko[2]), [o3] "v"(ko[3]), [o4] "v"(ko[4]), [o5] "v"(ko[5]), [o6] "v"(ko[6]), [o7] "v"(ko[7])
                                 : "memory");
                }
                // flags: 4 a next slot follows, 8 the next slot reads its A (else copies this one's)
                const int f = __builtin_amdgcn_readfirstlane((q + 1 < qb ? 4 : 0) | ((rlm >> (q + 1)) & 1 ? 8 : 0));
                const unsigned sna = q + 1 < NPW ? bufb + (__builtin_amdgcn_readlane(cur, 3 * q + 3) << 3) : 0u;
                const unsigned snb = q + 1 < NPW ? bufb + (__builtin_amdgcn_readlane(cur, 3 * q + 4) << 3) : 0u;
                asm volatile(
                    "s_waitcnt lgkmcnt(0)\n\t"
                    G64_MF(0)
                    "s_bitcmp0_b32 %[f], 2\n\t"
                    "s_cbranch_scc1 3f\n\t"
                    G64_RD("yb", "snb", 0, "t0") G64_RD("yb", "snb", 1, "t1") G64_MF(1)
                    G64_RD("yb", "snb", 2, "t0") G64_RD("yb", "snb", 3, "t1") G64_MF(2)
                    G64_RD("yb", "snb", 4, "t0") G64_RD("yb", "snb", 5, "t1") G64_MF(3)
                    G64_RD("yb", "snb", 6, "t0") G64_RD("yb", "snb", 7, "t1") G64_MF(4)
                    "s_bitcmp0_b32 %[f], 3\n\t"
                    "s_cbranch_scc1 2f\n\t"
                    G64_RD("ya", "sna", 0, "t0") G64_RD("ya", "sna", 1, "t1") G64_RD("ya", "sna", 2, "t0") G64_RD("ya", "sna", 3, "t1") G64_MF(5)
                    G64_RD("ya", "sna", 4, "t0") G64_RD("ya", "sna", 5, "t1") G64_RD("ya", "sna", 6, "t0") G64_RD("ya", "sna", 7, "t1") G64_MF(6)
                    G64_MF(7)
                    "s_branch 9f\n\t"
                    "2:\n\t"
                    G64_MV(0) G64_MV(1) G64_MV(2) G64_MV(3) G64_MF(5)
                    G64_MV(4) G64_MV(5) G64_MV(6) G64_MV(7) G64_MF(6)
                    G64_MF(7)
                    "s_branch 9f\n\t"
                    "3:\n\t"
                    G64_MF(1) G64_MF(2) G64_MF(3) G64_MF(4) G64_MF(5) G64_MF(6) G64_MF(7)
                    "9:"
                    : [acc] "+v"(acc[q]), [t0] "=&v"(t0), [t1] "=&v"(t1),
                      [xa0] "+v"(X[P][0]), [xa1] "+v"(X[P][1]), [xa2] "+v"(X[P][2]), [xa3] "+v"(X[P][3]),
                      [xa4] "+v"(X[P][4]), [xa5] "+v"(X[P][5]), [xa6] "+v"(X[P][6]), [xa7] "+v"(X[P][7]),
                      [xb0] "+v"(Y[P][0]), [xb1] "+v"(Y[P][1]), [xb2] "+v"(Y[P][2]), [xb3] "+v"(Y[P][3]),
                      [xb4] "+v"(Y[P][4]), [xb5] "+v"(Y[P][5]), [xb6] "+v"(Y[P][6]), [xb7] "+v"(Y[P][7]),
                      [ya0] "+v"(X[N][0]), [ya1] "+v"(X[N][1]), [ya2] "+v"(X[N][2]), [ya3] "+v"(X[N][3]),
                      [ya4] "+v"(X[N][4]), [ya5] "+v"(X[N][5]), [ya6] "+v"(X[N][6]), [ya7] "+v"(X[N][7]),
                      [yb0] "+v"(Y[N][0]), [yb1] "+v"(Y[N][1]), [yb2] "+v"(Y[N][2]), [yb3] "+v"(Y[N][3]),
                      [yb4] "+v"(Y[N][4]), [yb5] "+v"(Y[N][5]), [yb6] "+v"(Y[N][6]), [yb7] "+v"(Y[N][7])
                    : [f] "s"(f), [sna] "s"(sna), [snb] "s"(snb),
                      [o0] "v"(ko[0]), [o1] "v"(ko[1]), [o2] "v"(ko[2]), [o3] "v"(ko[3]), [o4] "v"(ko[4]), [o5] "v"(ko[5]), [o6] "v"(ko[6]), [o7] "v"(ko[7])
                    : "memory", "scc");
            }
#undef G64_RD
#undef G64_MF
#undef G64_MV
        }
    };
    int sg = 0;   // stage of step st
    long bh = 0;  // its block-half (of this workgroup's blocks)
    for (long st = 0; st < nst; st++) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of step st have landed
        __syncthreads();                                  // everyone's have; the other buffer is free
        const int sgn = sg + 1 == g.nstage ? 0 : sg + 1;
        const long bhn = sgn ? bh : bh + 1;
        if (st + 1 < nst) dma(sgn, bhn, (int)((st + 1) & 1));
        const double *buf = (st & 1) ? buf1 : buf0;
        const int lv0 = __builtin_amdgcn_readlane(svl, sg), lv1 = __builtin_amdgcn_readlane(svl, sg + 1);
        sg = sgn;
        bh = bhn;
        if constexpr (RUNS) {
            run_stage(buf, lv0, lv1);
            continue;
        }
        for (int lv = lv0; lv < lv1; lv++) {
            const int offv = slab[lv * g.NT + idxv];  // the slab offsets of all slots of the wave at this level: one LDS read
            int curI = -1;  // the tile whose operand the registers a[] hold (of this level)
            double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < NPW; q++) {
                const int tI = __builtin_amdgcn_readlane(mv, 3 * q), rg = __builtin_amdgcn_readlane(mv, 3 * q + 2);
                if (tI < 0 || lv < (rg & 0xff) || lv >= (rg >> 8)) continue;
                const double *pb = buf + __builtin_amdgcn_readlane(offv, 3 * q + 1);
                double b[NPW <= 10 ? 4 : 8];
                int p0 = p0c;
                if constexpr (NPW <= 10) asm volatile("" : "+v"(p0));  // (the 128-register shape: the eight positions are recomputed, not kept)
                if (tI != curI) {
                    const double *pa = buf + __builtin_amdgcn_readlane(offv, 3 * q);
#pragma unroll
                    for (int ks = 0; ks < 8; ks++) a[ks] = pa[p0 ^ (4 * ks)];
                    curI = tI;
                }
                // all operand reads of a group of k-steps are in flight before its first MFMA (the compiler would otherwise pair every MFMA
                // with the read in front of it and wait for each); the 128-register shape reads four k-steps at a time
                constexpr int KG = NPW <= 10 ? 4 : 8;
#pragma unroll
                for (int k0 = 0; k0 < 8; k0 += KG) {
#pragma unroll
                    for (int ks = k0; ks < k0 + KG; ks++) b[ks - k0] = pb[p0 ^ (4 * ks)];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int ks = k0; ks < k0 + KG; ks++) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b[ks - k0], acc[q], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    if constexpr (RUNS) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");  // (the asm MFMAs' results, before the stores read them)
#pragma unroll
    for (int q = 0; q < NPW; q++) {
        pp[q * 256 + 0 * 64 + lane] = acc[q][0];
        pp[q * 256 + 1 * 64 + lane] = acc[q][1];
        pp[q * 256 + 2 * 64 + lane] = acc[q][2];
        pp[q * 256 + 3 * 64 + lane] = acc[q][3];
    }
}
#endif
