// fbr_tsqr_plan.h -- host planning of the TSQR (fbr_tsqr_api.hip): column orders, row groups and the device tables of the row-group
// path.  HIP-free, so that tests/emul runs the library's own plan on the CPU.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "fbr_program.h"
#include "fbr_kinid.h"

// first column (in the order of the factorised columns) in which regressor row r can be non-zero: base-wrench rows meet every
// inertial column, the row of joint d the columns of the links below d and its own friction columns; Psel = only the rhs columns
static inline std::vector<int> tsqr_first_cols(const FbrHostModel &hm, const int32_t *cols, int Psel)
{
    std::vector<int> fc(hm.rows, Psel);
    for (int r = 0; r < hm.rows; r++)
        for (int c = 0; c < Psel; c++) {
            const FbrCol &cd = hm.coldesc[cols ? cols[c] : c];
            bool on;
            if (r < hm.fb)
                on = cd.kind == 0;
            else if (cd.kind == 0)
                on = std::find(hm.path[cd.link].begin(), hm.path[cd.link].end(), r - hm.fb) != hm.path[cd.link].end();
            else
                on = cd.joint == r - hm.fb;
            if (on) {
                fc[r] = c;
                break;
            }
        }
    return fc;
}

// Column order of a factorisation.  R^T R = A^T A holds for any column order of A, and a block of one regressor row is folded from
// the first column it can touch (tsqr_first_cols): with the inertial columns ordered by the DEPTH of their link (number of movable
// joints above it), every joint row starts behind all shallower links.  WALK-MAN: the folds run 0.44 instead of 0.55 of the dense
// tile updates and 0.60 instead of 0.71 of the panel chains.  The factor is computed in that order and brought back to the caller's
// column order by one small re-triangularisation (QR of the column-permuted n x n factor).  Friction columns keep their place behind
// the inertial ones.
struct TsqrPlan {
    int Psel = 0, Pa = 0;
    bool reorder = false;
    std::vector<int> fcols;    // [Psel] regressor column of factor column j
    std::vector<int> perm;     // [Pa]   caller's factor column of internal factor column j (rhs columns: identity)
    std::vector<int> inv;      // [Pa]   internal position of the caller's column j
    std::vector<int> linkpos;  // [L]    (all columns, no subset) block position of every link's columns
    std::vector<int> fc;       // [rows] first supported internal column of every regressor row
};
static inline long tsqr_plan_work(const std::vector<int> &fc, int n)
{
    long w = 0;
    const int NP = n / 16;
    for (int f : fc) {
        const long np_ = NP - std::min(f, n) / 16;
        w += np_ * (np_ - 1) / 2 + np_;
    }
    return w;
}
// narrow_cols: the widest padded factor of the wave-private kernels (16 x FBR_TSQR_NARROW_MAX_TILES), which never reorders
static inline TsqrPlan tsqr_plan(const FbrHostModel &hm, const int32_t *cols, int32_t ncols, int k, long S, bool allow_reorder, int narrow_cols)
{
    TsqrPlan p;
    p.Psel = cols ? ncols : hm.cols;
    p.Pa = p.Psel + k;
    const int n = (p.Pa + 15) & ~15;
    std::vector<int> ucols(p.Psel);
    for (int j = 0; j < p.Psel; j++) ucols[j] = cols ? cols[j] : j;
    std::vector<int> order(p.Psel);
    for (int j = 0; j < p.Psel; j++) order[j] = j;
    auto depth = [&](int j) { return hm.coldesc[ucols[j]].kind == 0 ? (int)hm.path[hm.coldesc[ucols[j]].link].size() : (1 << 20); };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return depth(a) < depth(b); });
    std::vector<int> sorted(p.Psel);
    for (int j = 0; j < p.Psel; j++) sorted[j] = ucols[order[j]];
    const std::vector<int> fc_user = tsqr_first_cols(hm, ucols.data(), p.Psel), fc_sorted = tsqr_first_cols(hm, sorted.data(), p.Psel);
    // worth it for wide factors and enough rows to pay for the final n x n re-triangularisation
    p.reorder = allow_reorder && n > narrow_cols && S * (long)hm.rows >= 64L * n &&
                tsqr_plan_work(fc_sorted, n) * 100 < tsqr_plan_work(fc_user, n) * 97;
    p.perm.resize(p.Pa);
    p.inv.resize(p.Pa);
    for (int j = 0; j < p.Pa; j++) p.perm[j] = (p.reorder && j < p.Psel) ? order[j] : j;
    for (int j = 0; j < p.Pa; j++) p.inv[p.perm[j]] = j;
    p.fcols = p.reorder ? sorted : ucols;
    p.fc = p.reorder ? fc_sorted : fc_user;
    if (!cols && !hm.masked) {
        p.linkpos.assign(hm.L, 0);
        for (int l = 0; l < hm.L; l++) p.linkpos[l] = p.inv[hm.cpl * l] / hm.cpl;
    }
    return p;
}

// ------------------------------------------------------------------------------------------------
// Tree-structured TSQR.  The row of joint d is non-zero only in the columns of the links below d (and its own friction columns), and
// R = qr(A) can be assembled from the factors of any partition of the ROWS.  The rows are therefore grouped along the kinematic
// tree -- the base-wrench rows, and one group per unbranched chain of joints (cut wherever the parent has more than one child joint)
// -- and every group is factorised over the columns its rows can touch only: WALK-MAN's leg joints fold 6 rows x 61 columns, its arm
// joints 7 x 81, the head 2 x 31, the waist 3 x 221 and only the 6 base rows all 481 (0.21 of the dense tile updates instead of the
// 0.44 of one factorisation with depth-ordered columns, and a third of the chunk bytes).  The group factors are embedded into the
// caller's column order and folded into the final factor like data rows.  Within a group the columns are ordered by link depth, so
// a joint row still starts at the first column of its own links.
// ------------------------------------------------------------------------------------------------
struct TsqrGroup {
    std::vector<int> rows;  // regressor rows of the group (slot order)
    std::vector<int> sel;   // factor columns of the group: indices into the caller's selected columns, in the group's order
    std::vector<int> fc;    // per slot: first supported column (group order)
    int Pa = 0;             // sel.size() + k
};
struct TsqrGroupPlan {
    std::vector<TsqrGroup> groups;
    std::vector<int> rowgroup, rowslot;  // per regressor row (-1: the row touches nothing that is factorised)
    bool masked = false;  // some regressor row has weight 0 for every sample and is left out
    int main = -1;  // group whose rows are dense in every factorised column (base-wrench rows): factorised in the caller's column order
                    // straight into the final factor, the other groups' factors are folded into it
};
static inline TsqrGroupPlan tsqr_group_plan(const FbrHostModel &hm, const int32_t *cols, int32_t ncols, int k, const std::vector<char> *active = nullptr,
                                            bool m_force_group = true)
{
    TsqrGroupPlan gp;
    const int Psel = cols ? ncols : hm.cols;
    // joint tree: parent joint of joint d (-1: hangs off the base), number of child joints of every joint (index 0: the base)
    std::vector<int> pj(hm.n, -1), depth(hm.n, 0), nchild(hm.n + 1, 0);
    for (int l = 0; l < hm.L; l++) {
        const int d = hm.dof[l];
        if (d < 0) continue;
        const std::vector<int> &pa = hm.path[l];
        depth[d] = (int)pa.size();
        pj[d] = pa.size() >= 2 ? pa[pa.size() - 2] : -1;
    }
    for (int d = 0; d < hm.n; d++) nchild[pj[d] + 1]++;
    std::vector<int> jgroup(hm.n, -1);
    int ngroups = 0, base_group = -1;
    if (hm.fb) base_group = ngroups++;
    std::vector<int> order(hm.n);
    for (int d = 0; d < hm.n; d++) order[d] = d;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return depth[a] < depth[b]; });
    for (int d : order) {
        const int p = pj[d];
        int pg = p < 0 ? base_group : jgroup[p];
        if (nchild[p + 1] == 1 && pg < 0) pg = base_group = ngroups++;  // fixed base, single chain from the root
        jgroup[d] = (nchild[p + 1] == 1) ? pg : ngroups++;
    }
    // The FORCE rows of the base wrench (rows 0 .. 2 of a floating base) are non-zero only in the columns that produce a force -- a link's
    // mass and first moments (an inertia entry is a pure moment) --: a group of their own, factorised over those columns (WALK-MAN, regrouped:
    // 62 of 213), leaves the dense group the three moment rows: the widest group folds half the rows (round 6; option tsqr_force_group)
    const bool force_split = hm.fb == 6 && m_force_group;
    const int force_group = force_split ? ngroups++ : -1;
    std::vector<std::vector<int>> grows(ngroups);
    auto on = [&](int r) { return !active || (*active)[r]; };  // rows switched off by the weights belong to no group
    for (int r = 0; r < hm.fb; r++)
        if (on(r)) grows[(force_split && r < 3) ? force_group : base_group].push_back(r);
    for (int d = 0; d < hm.n; d++)
        if (on(hm.fb + d)) grows[jgroup[d]].push_back(hm.fb + d);
    for (int r = 0; r < hm.rows; r++) gp.masked = gp.masked || !on(r);
    auto touches = [&](int r, int uc) {
        const FbrCol &cd = hm.coldesc[uc];
        if (cd.kind != 0) return cd.joint == r - hm.fb;
        if (force_split && r < 3) return cd.pidx < 4;
        if (r < hm.fb) return true;
        const std::vector<int> &pa = hm.path[cd.link];
        return std::find(pa.begin(), pa.end(), r - hm.fb) != pa.end();
    };
    gp.rowgroup.assign(hm.rows, -1);
    gp.rowslot.assign(hm.rows, -1);
    for (int g = 0; g < ngroups; g++) {
        TsqrGroup G;
        if (grows[g].empty()) continue;
        std::vector<int> inert, fric;
        for (int j = 0; j < Psel; j++) {
            const int uc = cols ? cols[j] : j;
            bool any = false;
            for (int r : grows[g]) any = any || touches(r, uc);
            if (any) (hm.coldesc[uc].kind == 0 ? inert : fric).push_back(j);
        }
        // (the unpaired columns of a model with column masks go behind the paired ones: pairs stay at even positions in every group)
        auto cdepth = [&](int j) {
            const FbrCol &cd = hm.coldesc[cols ? cols[j] : j];
            return (int)hm.path[cd.link].size() + (cd.joint == -2 ? (1 << 16) : 0);
        };
        std::stable_sort(inert.begin(), inert.end(), [&](int a, int b) { return cdepth(a) < cdepth(b); });
        G.sel = inert;
        G.sel.insert(G.sel.end(), fric.begin(), fric.end());
        G.Pa = (int)G.sel.size() + k;
        if (G.Pa == 0) continue;
        // slots: rows with the widest support first (their blocks start at the left-most panels)
        G.rows = grows[g];
        auto first = [&](int r) {
            for (size_t i = 0; i < G.sel.size(); i++)
                if (touches(r, cols ? cols[G.sel[i]] : G.sel[i])) return (int)i;
            return (int)G.sel.size();
        };
        std::stable_sort(G.rows.begin(), G.rows.end(), [&](int a, int b) { return first(a) < first(b); });
        bool dense = (int)G.sel.size() == Psel;
        for (size_t i = 0; i < G.rows.size(); i++) {
            G.fc.push_back(first(G.rows[i]));
            dense = dense && G.fc.back() == 0;
            gp.rowgroup[G.rows[i]] = (int)gp.groups.size();
            gp.rowslot[G.rows[i]] = (int)i;
        }
        if (dense && gp.main < 0) {
            gp.main = (int)gp.groups.size();
            std::sort(G.sel.begin(), G.sel.end());  // = the caller's order
        }
        gp.groups.push_back(std::move(G));
    }
    return gp;
}

// Device tables of a row-group call: one int table (offsets o_*), the writer entry lists and the lane writer's destination slots.  An
// entry is (regressor row | kind << 8 | column position in the row's group << 10), kind 0 base row, 1 joint row on the link's path, 2
// structural zero, 3 friction column of the row's joint.
struct TsqrGroupTables {
    std::vector<int> tab;
    size_t o_ebeg[2] = {0, 0}, o_pbeg[2] = {0, 0};  // per model column (pair): first entry, variant 0 / 1
    size_t o_lrec = 0, o_lcol = 0, o_lsteps = 0;     // lane writer: (first slot, zero entries) per column, columns per part and link, steps
    size_t o_rowoff = 0;                             // per regressor row: offset in a sample's LDS image (filled in by the caller)
    size_t o_nrows = 0, o_gpa = 0;                   // per group: slots, columns (rhs included)
    std::vector<size_t> o_fc, o_emb;                 // per group: slot first columns, embedding into the caller's columns (Pa)
    std::vector<int> ents[2], pents[2];              // entry lists; pair entry lists (empty unless pairable)
    int npairs = 0, wsplit = 1;
    bool pairable = false;
    bool lane_writer = false;
    size_t lane_lds = 0;
    std::vector<std::pair<int, int>> lslots;  // per destination slot of the lane writer: (regressor row, column position), row -1: absent
    int lane_parts = 1, lane_slots = 1, lane_step0[FBR_KINWRITE_PARTS] = {0, 0, 0, 0}, lane_nsteps[FBR_KINWRITE_PARTS] = {0, 0, 0, 0};
};
// tsqr_writer / lane_writer: the options of that name; has_kinid: the model has a fused kinematic program
static inline TsqrGroupTables tsqr_group_tables(const FbrHostModel &hm, const TsqrGroupPlan &gp, const int32_t *cols, int Psel, int k, bool has_w,
                                                int tsqr_writer, bool lane_writer, bool has_kinid)
{
    TsqrGroupTables T;
    std::vector<int> &tab = T.tab;
    std::vector<int>(&ents)[2] = T.ents, (&pents)[2] = T.pents;
    const int G = (int)gp.groups.size(), Pa = Psel + k;
    tab.insert(tab.end(), gp.rowgroup.begin(), gp.rowgroup.end());
    tab.insert(tab.end(), gp.rowslot.begin(), gp.rowslot.end());
    // what every model column writes: one entry per row of every group that holds the column (variant 1: without the structural zeros
    // left of the row's first supported column tile)
    std::vector<int> gposv((size_t)G * hm.cols, -1);
    for (int g = 0; g < G; g++)
        for (size_t i = 0; i < gp.groups[g].sel.size(); i++) {
            const int j = gp.groups[g].sel[i];
            gposv[(size_t)g * hm.cols + (cols ? cols[j] : j)] = (int)i;
        }
    for (int var = 0; var < 2; var++) {
        T.o_ebeg[var] = tab.size();
        for (int c = 0; c < hm.cols; c++) {
            tab.push_back((int)ents[var].size());
            const FbrCol &cd = hm.coldesc[c];
            for (int r = 0; r < hm.rows; r++) {
                const int g = gp.rowgroup[r];
                if (g < 0) continue;
                const int pos = gposv[(size_t)g * hm.cols + c];
                if (pos < 0) continue;
                int kind;
                if (cd.kind == 0) {
                    if (r < hm.fb)
                        kind = 0;
                    else {
                        const std::vector<int> &pa = hm.path[cd.link];
                        kind = std::find(pa.begin(), pa.end(), r - hm.fb) != pa.end() ? 1 : 2;
                    }
                } else {
                    kind = cd.joint == r - hm.fb ? 3 : 2;
                }
                const int slot = gp.rowslot[r];
                if (var == 1 && kind == 2 && pos < (gp.groups[g].fc[slot] & ~15)) continue;
                ents[var].push_back(r | (kind << 8) | (pos << 10));
            }
        }
        tab.push_back((int)ents[var].size());
    }
    // the same lists per PAIR of adjacent inertial columns (16-byte stores, fbr_regressor_groups2_kernel): possible when both columns
    // of every pair sit side by side at an even position in every group that holds them
    const int npairs = T.npairs = hm.npaircols / 2;
    // threads per work item of the pair writer (fbr_regressor_groups2_kernel: 256 threads, an item's entries dealt to `wsplit` of them)
    T.wsplit = std::max(1, std::min(4, 256 / std::max(1, npairs + (hm.cols - 2 * npairs))));
    // (with fewer work items than half a workgroup -- the regrouped WALK-MAN: 92 pairs + 29 single columns -- the pair writer leaves
    // most threads idle behind twice the work per busy thread: 12.6 ms per 1 M samples with the entries split, 15.9 without, against
    // 11.8 ms of the one-column-per-thread writer)
    bool pairable = npairs > 0 && tsqr_writer != 8 && (npairs + (hm.cols - 2 * npairs) >= 128 || tsqr_writer == 16);
    for (int var = 0; var < 2 && pairable; var++) {
        T.o_pbeg[var] = tab.size();
        for (int pr = 0; pr < npairs && pairable; pr++) {
            tab.push_back((int)pents[var].size());
            const int c = 2 * pr;
            const int ea = tab[T.o_ebeg[var] + c], eb = tab[T.o_ebeg[var] + c + 1], ec = tab[T.o_ebeg[var] + c + 2];
            pairable = hm.coldesc[c].kind == 0 && hm.coldesc[c + 1].kind == 0 && hm.coldesc[c].link == hm.coldesc[c + 1].link && eb - ea == ec - eb;
            for (int i = 0; i < eb - ea && pairable; i++) {
                const int x = ents[var][ea + i], y = ents[var][eb + i];
                pairable = (x & 0x3ff) == (y & 0x3ff) && (y >> 10) == (x >> 10) + 1 && ((x >> 10) & 1) == 0;
                pents[var].push_back(x);
            }
        }
        tab.push_back((int)pents[var].size());
    }
    T.pairable = pairable;
    if (!pairable) pents[0].clear(), pents[1].clear();
    // ---- the lane writer (fbr_kinid.h fbr_kinwrite_kernel, option tsqr_lane_writer): one lane per sample, kinematics fused in, chunks
    // written column-major.  Its entries carry the level of the row's joint on the link's path instead of a motion-vector lookup.
    T.lane_lds = ((size_t)3 * 64 * (std::max(hm.n, 1) | 1) + (has_w ? (size_t)64 * (hm.rows | 1) : 0)) * sizeof(double);
    T.lane_writer = lane_writer && tsqr_writer == 0 && has_kinid && T.lane_lds <= (size_t)(120 << 10) && Pa < 1024;
    if (T.lane_writer) {
        std::vector<std::pair<int, int>> &lslots = T.lslots;
        T.o_lrec = tab.size();
        auto entry_of = [&](int c, int r, int kind, int *pos) {  // the writer entry (variant 1) of column c on row r, if any
            for (int e = tab[T.o_ebeg[1] + c]; e < tab[T.o_ebeg[1] + c + 1]; e++)
                if ((ents[1][e] & 0xff) == r && ((ents[1][e] >> 8) & 3) == kind) {
                    *pos = ents[1][e] >> 10;
                    return true;
                }
            return false;
        };
        for (int c = 0; c < hm.cols; c++) {
            const FbrCol &cd = hm.coldesc[c];
            if (tab[T.o_ebeg[1] + c] == tab[T.o_ebeg[1] + c + 1]) {  // no group holds the column
                tab.push_back(-1);
                tab.push_back(0);
                continue;
            }
            tab.push_back((int)lslots.size());
            int pos = 0, nz = 0;
            if (cd.kind == 0) {
                for (int r = 0; r < hm.fb; r++) lslots.push_back(entry_of(c, r, 0, &pos) ? std::make_pair(r, pos) : std::make_pair(-1, 0));
                for (int dj : hm.path[cd.link]) lslots.push_back(entry_of(c, hm.fb + dj, 1, &pos) ? std::make_pair(hm.fb + dj, pos) : std::make_pair(-1, 0));
            } else {
                lslots.push_back(entry_of(c, hm.fb + cd.joint, 3, &pos) ? std::make_pair(hm.fb + cd.joint, pos) : std::make_pair(-1, 0));
            }
            for (int e = tab[T.o_ebeg[1] + c]; e < tab[T.o_ebeg[1] + c + 1]; e++)
                if (((ents[1][e] >> 8) & 3) == 2) {
                    lslots.push_back({ents[1][e] & 0xff, ents[1][e] >> 10});
                    nz++;
                }
            tab.push_back(nz);
        }
        tab.push_back((int)lslots.size());  // pseudo-column `cols`: k rhs destinations per regressor row
        tab.push_back(0);
        for (int r = 0; r < hm.rows; r++)
            for (int i = 0; i < k; i++)
                lslots.push_back(gp.rowgroup[r] >= 0 ? std::make_pair(r, (int)gp.groups[gp.rowgroup[r]].sel.size() + i) : std::make_pair(-1, 0));
        // the tree in parts: the waves of a workgroup share one block of samples, each walks its links (+ the ancestors they need) and
        // writes the columns of its own links (fbr_kinid_build_parts); cost of a link: its kinematics + what its columns write
        std::vector<double> lcost(hm.L, 30.0);
        for (int c = 0; c < hm.ninert; c++)
            if (tab[T.o_lrec + 2 * c] >= 0) lcost[hm.coldesc[c].link] += 10.0 + (double)(hm.fb + hm.path[hm.coldesc[c].link].size() + tab[T.o_lrec + 2 * c + 1]);
        std::vector<FbrKinIdProgram> progs;
        std::vector<std::vector<char>> own;
        fbr_kinid_build_parts(hm, lcost, FBR_KINWRITE_PARTS, progs, own);
        T.lane_parts = (int)progs.size();
        T.o_lcol = tab.size();
        tab.resize(tab.size() + (size_t)T.lane_parts * 10 * hm.L, -1);
        for (int c = 0; c < hm.ninert; c++)
            for (int pq = 0; pq < T.lane_parts; pq++)
                if (own[pq][hm.coldesc[c].link]) tab[T.o_lcol + (size_t)pq * 10 * hm.L + 10 * hm.coldesc[c].link + hm.coldesc[c].pidx] = c;
        T.o_lsteps = tab.size();
        for (int pq = 0; pq < T.lane_parts; pq++) {
            T.lane_step0[pq] = (int)((tab.size() - T.o_lsteps) / FBR_KINID_STEP);
            T.lane_nsteps[pq] = progs[pq].nsteps;
            T.lane_slots = std::max(T.lane_slots, progs[pq].nslots);
            tab.insert(tab.end(), progs[pq].steps.begin(), progs[pq].steps.begin() + (size_t)progs[pq].nsteps * FBR_KINID_STEP);
        }
    }
    // LDS image of one sample's rows (fbr_regressor_groups_lds_kernel): offset of regressor row r, ld_g doubles each -- the padded width
    // of a group is only known once its factorisation has begun: the caller fills the offsets in
    T.o_rowoff = tab.size();
    tab.resize(tab.size() + hm.rows, -1);
    T.o_nrows = tab.size();
    for (int g = 0; g < G; g++) tab.push_back((int)gp.groups[g].rows.size());
    T.o_gpa = tab.size();
    for (int g = 0; g < G; g++) tab.push_back(gp.groups[g].Pa);
    T.o_fc.resize(G);
    T.o_emb.resize(G);
    for (int g = 0; g < G; g++) {
        T.o_fc[g] = tab.size();
        tab.insert(tab.end(), gp.groups[g].fc.begin(), gp.groups[g].fc.end());
    }
    for (int g = 0; g < G; g++) {
        // column j of the final factor (caller's order) <- column emb[j] of the group factor, -1: not in the group
        T.o_emb[g] = tab.size();
        tab.resize(tab.size() + Pa, -1);
        const TsqrGroup &Gg = gp.groups[g];
        for (size_t i = 0; i < Gg.sel.size(); i++) tab[T.o_emb[g] + Gg.sel[i]] = (int)i;
        for (int i = 0; i < k; i++) tab[T.o_emb[g] + Psel + i] = (int)Gg.sel.size() + i;
    }
    while (tab.size() & 3) tab.push_back(0);
    return T;
}
