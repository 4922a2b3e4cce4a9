// fbr_tsqr_api.hip -- blocked Householder TSQR of libfbr (fbr_tsqr / _cols / _submit / _merge / _work_info, include/fbr.h; kernels in fbr_tsqr.h).
#define FBR_KERNELS_GROUPS
#include "fbr_internal.h"
#include "fbr_tsqr.h"
#include "fbr_tsqr_plan.h"

// ------------------------------------------------------------------------------------------------
// TSQR (fbr_tsqr.h)
// ------------------------------------------------------------------------------------------------
static FbrTsqrOpts topts(const fbr_model *m)
{
    FbrTsqrOpts o;
    o.narrow = m->opt.tsqr_narrow != 0;
    o.tree_one_wg = m->opt.tsqr_tree_one_wg != 0;
    o.timing = m->opt.tsqr_timing != 0;
    o.short_calls = m->opt.tsqr_short_call_factors != 0;
    o.narrow_tall = m->opt.tsqr_narrow_tall != 0;
    return o;
}
// fbr_tsqr_begin with the model's options
static int tsqr_begin(const fbr_model *m, FbrTsqrWork &wk, hipStream_t st, int Pa, const double *R_in, int num_cus, long rows_hint, unsigned *shared_err = nullptr)
{
    wk.opts = topts(m);
    return fbr_tsqr_begin(wk, st, Pa, R_in, num_cus, rows_hint, shared_err);
}

// groups pay when the tree branches and there are enough rows to keep every group's workers busy
static bool tsqr_use_groups(const fbr_model *m, const TsqrGroupPlan &gp, long S)
{
    const long min_s = (long)m->opt.tsqr_group_min_samples;  // (tests force the path at small sizes) default 24000: measured on WALK-MAN, groups vs one factorisation: 16 k samples 16 vs 15.8 ms, 32 k 18.5 vs 21.4, 64 k 24 vs 32, 125 k 34 vs 52
    // (a chain on a FIXED base has ONE group and keeps the plain path; on a floating base the force rows are a second group -- tsqr_force_group --
    // and the call takes the row-group path: left arm 500 k samples 3.8 instead of 7.3 ms.  Measured, round 6, with ONE group: sending it through the row-group path for the sake
    // of the lane writer -- column-major chunks -- costs the wave-private level-0 kernel more than the writer saves: left arm 500 k samples
    // 8.5 instead of 7.3 ms (folds 6.6 instead of 5.7 ms: one wave per SIMD cannot hide the 16-lines-per-instruction block loads), KUKA 4.07
    // instead of 4.23)
    return (gp.groups.size() > 1 || (gp.masked && !gp.groups.empty())) && S >= min_s && m->opt.tsqr_groups != 0;
}
// Samples per chunk of a call over S samples, and (*lcm_out) the block granularity: every chunk is a whole number of fold blocks per
// regressor row in every group.  The chunks are cut EVENLY (a call that exceeds the memory-sized chunk by a few samples used to end with
// a chunk of a handful of samples that cost a dozen launches: 0.66 of the 10.3 ms of a 125 k-sample WALK-MAN call), a call up to 5 %
// longer than one chunk stays one chunk, and the last chunk is padded to the granularity with zero rows (tsqr_write_chunk).
static long tsqr_group_chunk_samples(const fbr_model *m, const TsqrGroupPlan &gp, long S, long *lcm_out = nullptr)
{
    double per = 0.0;  // chunk bytes per sample over all groups
    long lcm = 1;
    for (const TsqrGroup &G : gp.groups) {
        FbrTsqrShape sh;
        if (fbr_tsqr_shape(G.Pa, m->num_cus, 1L << 40, &sh, topts(m))) return -1;
        per += 8.0 * (double)G.rows.size() * sh.n;
        lcm = std::lcm(lcm, (long)sh.mb);
    }
    long ch = std::max(1L, (long)(4.0 * 1024 * 1024 * 1024 / per));
    ch = std::min(ch, chunk_size(m, 1L << 40));  // (the memory-sized chunk; chunk_size caps at the call's own length otherwise)
    // (an oversized chunk_samples costs memory only: the level-0 folds address a block's first row in 64 bits, r0 * n or r0 + c * cs,
    // and the 32-bit products inside a block, row * ldb of fbr_tsqr.h, stay below MB * FBR_TSQR_MAXN whatever the chunk length; the lane
    // writer's 32-bit lane offset, sample << 3 in fbr_kinwrite_kernel, wraps only at 2^29 samples per chunk, 4 GiB per regressor row and
    // column of the chunk, which no allocation of the chunk holds)
    if (m->opt.chunk_samples >= 1) ch = (long)m->opt.chunk_samples;
    ch = std::max(lcm, ch - ch % lcm);
    if (lcm_out) *lcm_out = lcm;
    if (S <= 0) return ch;
    const long nch = std::max(1L, (long)std::ceil((double)S / (1.05 * (double)ch)));
    const long even = (S + nch - 1) / nch;
    return (even + lcm - 1) / lcm * lcm;  // whole blocks per slot in every group
}

// Device tables of a TSQR call: assembled in pinned host memory that belongs to the call's ticket parity and copied asynchronously on
// `st` -- no host wait, and the tables of the submission before (other parity) stay intact while it is still running.
static int tsqr_upload_tables(fbr_model *m, int par, const std::vector<std::pair<const void *, size_t>> &pieces, const std::vector<size_t> &offs,
                              size_t total, hipStream_t st, const char **dev)
{
    total = std::max<size_t>(total, 16);
    if (m->tsqr_tab_host_bytes[par] < total) {
        if (m->tsqr_tab_host[par]) (void)hipHostFree(m->tsqr_tab_host[par]);
        m->tsqr_tab_host[par] = nullptr;
        m->tsqr_tab_host_bytes[par] = 0;
        HIPCHK(hipHostMalloc(&m->tsqr_tab_host[par], total + total / 2, hipHostMallocDefault));
        m->tsqr_tab_host_bytes[par] = total + total / 2;
    }
    int rc = m->tsqr_tab[par].ensure(total);
    if (rc) return rc;
    for (size_t i = 0; i < pieces.size(); i++)
        if (pieces[i].second) memcpy((char *)m->tsqr_tab_host[par] + offs[i], pieces[i].first, pieces[i].second);
    HIPCHK(hipMemcpyAsync(m->tsqr_tab[par].p, m->tsqr_tab_host[par], total, hipMemcpyHostToDevice, st));
    *dev = (const char *)m->tsqr_tab[par].p;
    return FBR_OK;
}

// fbr_tsqr_* return code -> FBR_E_*, with the TSQR layer's message behind `what`
static int tsqr_status(int code, const char *what)
{
    set_err(std::string(what) + ": " + fbr_tsqr_error());
    return code == -4 ? FBR_E_UNSUPPORTED : (code == -3 ? FBR_E_HIP : FBR_E_INVALID);
}

constexpr int TSQR_NSIDE = (int)(sizeof(fbr_model::tsqr_streams) / sizeof(fbr_model::tsqr_streams[0]));

// One row-group call (tsqr_groups_impl): what its phases share
struct TsqrGroupCall {
    fbr_model *m;
    const DevStates &d;
    const TsqrGroupPlan &gp;
    TsqrGroupTables tt;
    const double *drhs, *dw;
    int k, Pa;
    long ch, lcm;                   // samples per chunk, block granularity (tsqr_group_chunk_samples)
    std::vector<FbrDevGroup> hg;    // per group: chunk buffer, its leading dimension, columns
    int img_total = 0;              // doubles of a sample's LDS image (the LDS-staged writer)
    size_t lds = 0, lds_img = 0;    // dynamic LDS of the writers, of the LDS-staged one
    bool lds_writer = false;
    long csp_of[2] = {0, 0};        // rows per slot of the full chunks and of the last one
    const char *dtab = nullptr;     // the tables on the device: tt.tab, then (byte offsets) the entry lists of variant 1, the pair entry
    const int *t = nullptr;         // lists of variant 1, the groups' records and the lane writer's two destination sets of nlent each
    size_t o_ent1 = 0, o_pent1 = 0, o_lent = 0, nlent = 0;
    const FbrDevGroup *dgrp = nullptr;
    double *rtmp = nullptr;         // the groups' factors, Pa x Pa each at o_r
    std::vector<size_t> o_r;
    std::vector<int> side_order;    // the groups other than the main one, the longest trees first
    FbrTsqrWork &work(int g) const { return g == gp.main ? m->tsqr : m->tsqr_groups[g]; }
};

// The streams and events of the row-group path (created on first use)
static int ensure_tsqr_streams(fbr_model *m, bool overlap)
{
    // prologue stream: everything up to the first chunk's writer
    // (a stream confined to three quarters of the CUs: the prologue's kernels would otherwise fill every CU with their waves, and the
    // tree's eight-wave workgroups -- a whole CU's registers each -- could not be placed until they drain: measured, the first tree
    // level then takes 3.6 instead of 1.0 ms and nothing is gained)
    if (overlap && !m->tsqr_pro_stream) {
        const int words = (m->num_cus + 31) / 32;
        std::vector<uint32_t> mask(words, 0x00ffffffu);
        if (hipExtStreamCreateWithCUMask(&m->tsqr_pro_stream, (uint32_t)words, mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            HIPCHK(hipStreamCreateWithFlags(&m->tsqr_pro_stream, hipStreamNonBlocking));
        }
    }
    // the side streams get DIFFERENT priority levels: HIP gives a stream of another level a hardware queue of its own, while streams of
    // one level share a few queues round robin -- three trees on two queues were the tail of the call (the legs' tree queued behind
    // the arms')
    for (int i = 0; i < TSQR_NSIDE; i++)
        if (!m->tsqr_streams[i]) {
            int least = 0, greatest = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
            const int prios[4] = {greatest, least, (least + greatest) / 2, (least + greatest) / 2};
            HIPCHK(hipStreamCreateWithPriority(&m->tsqr_streams[i], hipStreamNonBlocking, prios[i]));
        }
    for (auto &e : m->tsqr_ev)
        if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return FBR_OK;
}

// Begins the groups' factorisations on the main stream -- the main group's is the final factor: it also folds the other groups' factors
// -- and takes their chunk buffers on the prologue stream pst (cleared unless the lane writer writes every element of them)
static int tsqr_begin_groups(TsqrGroupCall &c, const double *Rin_dev, hipStream_t pst, bool overlap)
{
    fbr_model *m = c.m;
    const TsqrGroupPlan &gp = c.gp;
    const int G = (int)gp.groups.size();
    const long S = c.d.S;
    int rc;
    long mrows = 0;  // rows the final factor folds: the main group's data rows and the other groups' factors
    for (int g = 0; g < G; g++) mrows += g == gp.main ? S * (long)gp.groups[g].rows.size() : gp.groups[g].Pa;
    for (int g = 0; g < G; g++) {
        const TsqrGroup &Gg = gp.groups[g];
        if ((rc = tsqr_begin(m, c.work(g), m->stream, Gg.Pa, g == gp.main ? Rin_dev : nullptr, m->num_cus, g == gp.main ? mrows : S * (long)Gg.rows.size(),
                             m->tsqr_err)))
            return tsqr_status(rc, "tsqr group begin");
    }
    if (overlap) HIPCHK(hipStreamWaitEvent(pst, m->ev_tsqr_l0, 0));  // the chunk buffers and the kinematic records are free again
    c.hg.resize(G);
    for (int g = 0; g < G; g++) {
        FbrTsqrWork &wk = c.work(g);
        double *A = nullptr;
        if ((rc = fbr_tsqr_chunk_buffer(wk, c.ch * (long)gp.groups[g].rows.size(), &A)) || (!c.tt.lane_writer && (rc = fbr_tsqr_chunk_clean(wk, pst))))
            return tsqr_status(rc, "tsqr group chunk");
        c.hg[g] = FbrDevGroup{A, wk.n, (int)gp.groups[g].sel.size()};
    }
    for (int r = 0; r < m->hm.rows; r++)  // a sample's LDS image: ld_g doubles per row
        if (gp.rowgroup[r] >= 0) {
            c.tt.tab[c.tt.o_rowoff + r] = c.img_total;
            c.img_total += c.hg[gp.rowgroup[r]].ld;
        }
    return FBR_OK;
}

// The dynamic LDS of the record writers.  The LDS-staged writer (option tsqr_writer = 32) needs a sample's rows to fit a third of the LDS
// beside the record.
static int tsqr_writer_setup(TsqrGroupCall &c)
{
    const fbr_model *m = c.m;
    const FbrHostModel &hm = m->hm;
    const int naux = hm.rows * c.k + (c.dw ? hm.rows : 0) + (hm.fric ? hm.n : 0) + ((hm.fric && c.d.sign) ? hm.n : 0);
    c.lds_img = ((size_t)((hm.rec_size() + 1) & ~1) + ((naux + 1) & ~1) + ((hm.rows + 1) & ~1) + c.img_total) * sizeof(double) +
                (size_t)((c.img_total / 2 + 3) & ~3) * sizeof(unsigned short) + ((size_t)3 * hm.rows + c.tt.ents[1].size()) * sizeof(int);
    // (measured, round 5, regrouped WALK-MAN: the call of 1 M samples 54.95 instead of 55.88 ms, of 125 k samples 9.86 instead of 9.52 ms --
    // the writer is not bound by the width of its stores; the staged writer is therefore an option, not the default)
    c.lds_writer = m->opt.tsqr_writer == 32 && hm.rows <= 255 && c.img_total > 0 && c.lds_img <= 64 * 1024 && hm.rec_size() <= 256 * 6 && naux <= 512 &&
                   hm.cols <= 512;
    if (m->opt.tsqr_writer == 32 && !c.lds_writer) {
        set_err("tsqr_writer = 32: the rows of a sample do not fit the LDS image of the staged writer");
        return FBR_E_UNSUPPORTED;
    }
    c.lds = (size_t)((hm.rec_size() + 1) & ~1) * sizeof(double) + (size_t)hm.rows * sizeof(double *);
    HIPCHK(hipFuncSetAttribute((const void *)fbr_regressor_groups_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds));
    HIPCHK(hipFuncSetAttribute((const void *)fbr_regressor_groups2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds));
    if (c.lds_writer) HIPCHK(hipFuncSetAttribute((const void *)fbr_regressor_groups_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds_img));
    return FBR_OK;
}

// Uploads the tables on the prologue stream.  The lane writer's column stride is fixed per chunk, its row pointers are rebuilt per chunk
// on the device side of the tables: set 0 for the full chunks (ch samples per slot), set 1 for the last chunk (padded to the granularity).
// An entry's destination is the address of (its row's slot, sample 0, its column) in the column-major chunk of the row's group.
static int tsqr_upload_group_tables(TsqrGroupCall &c, int par, hipStream_t pst)
{
    const TsqrGroupTables &tt = c.tt;
    const TsqrGroupPlan &gp = c.gp;
    const int G = (int)gp.groups.size();
    const long S = c.d.S;
    const size_t o_ent0 = tt.tab.size() * sizeof(int);
    c.o_ent1 = o_ent0 + tt.ents[0].size() * sizeof(int);
    const size_t o_pent0 = c.o_ent1 + tt.ents[1].size() * sizeof(int);
    c.o_pent1 = o_pent0 + tt.pents[0].size() * sizeof(int);
    const size_t o_grp = (c.o_pent1 + tt.pents[1].size() * sizeof(int) + 15) & ~(size_t)15;
    const size_t nlent = c.nlent = tt.lslots.size() + 64;  // (padded: the kernel requests a record's destinations in fixed-size batches)
    c.o_lent = (o_grp + (size_t)G * sizeof(FbrDevGroup) + 15) & ~(size_t)15;
    std::vector<long long> lane_dst(2 * nlent, 0);
    const long last_cs = S > 0 ? S - (S - 1) / c.ch * c.ch : 0;
    c.csp_of[0] = c.ch;
    c.csp_of[1] = (last_cs + c.lcm - 1) / c.lcm * c.lcm;
    if (tt.lane_writer)
        for (int j = 0; j < 2; j++)
            for (size_t e = 0; e < tt.lslots.size(); e++) {
                const int r = tt.lslots[e].first, pos = tt.lslots[e].second;
                if (r < 0) continue;
                const int g = gp.rowgroup[r];
                const long ldc = (long)gp.groups[g].rows.size() * c.csp_of[j];
                lane_dst[j * nlent + e] = (long long)(uintptr_t)(c.hg[g].A + (long)pos * ldc + (long)gp.rowslot[r] * c.csp_of[j]);
            }
    if (int rc = tsqr_upload_tables(c.m, par,
                                    {{tt.tab.data(), tt.tab.size() * sizeof(int)}, {tt.ents[0].data(), tt.ents[0].size() * sizeof(int)},
                                     {tt.ents[1].data(), tt.ents[1].size() * sizeof(int)}, {tt.pents[0].data(), tt.pents[0].size() * sizeof(int)},
                                     {tt.pents[1].data(), tt.pents[1].size() * sizeof(int)}, {c.hg.data(), G * sizeof(FbrDevGroup)},
                                     {lane_dst.data(), lane_dst.size() * sizeof(long long)}},
                                    {0, o_ent0, c.o_ent1, o_pent0, c.o_pent1, o_grp, c.o_lent}, c.o_lent + lane_dst.size() * sizeof(long long), pst, &c.dtab))
        return rc;
    c.t = (const int *)c.dtab;
    c.dgrp = (const FbrDevGroup *)(c.dtab + o_grp);
    return FBR_OK;
}

// Writes the samples [s0, s0 + cs) into the groups' chunk buffers, csp >= cs rows per slot, on stream cst: the lane writer (kinematics
// fused in), or the kinematic records and then the LDS-staged, the pair or the one-column writer
static int tsqr_write_chunk(TsqrGroupCall &c, long s0, long cs, long csp, hipStream_t cst)
{
    fbr_model *m = c.m;
    const DevStates &d = c.d;
    const FbrHostModel &hm = m->hm;
    const TsqrGroupTables &tt = c.tt;
    const int G = (int)c.gp.groups.size(), k = c.k, *t = c.t;
    const long S = d.S, ch = c.ch;
    const double *drhs = c.drhs, *dw = c.dw;
    int rc;
    size_t maxrows = 1;
    for (int g = 0; g < G; g++) maxrows = std::max(maxrows, c.gp.groups[g].rows.size());
    if (tt.lane_writer) {
        // one kernel: kinematics + every entry of the groups' chunks, column-major (512-byte runs); padding rows / columns cleared first
        hipLaunchKernelGGL(fbr_groups_clear_cm_kernel, dim3(G, (unsigned)maxrows + FBR_CM_PADWG), dim3(256), 0, cst, c.dgrp, t + tt.o_nrows, t + tt.o_gpa, cs, csp,
                           (int)maxrows);
        HIPCHK(hipGetLastError());
        const int set = (csp == c.csp_of[0] && cs == ch) ? 0 : 1;
        if (csp != c.csp_of[set]) {
            set_err("internal: chunk stride of the lane writer does not match its row tables");
            return FBR_E_INVALID;
        }
        const DevKinId kp = kinid_params(m, m->kinid.nsteps, tt.lane_slots, t + tt.o_lsteps);
        DevKinWrite kw{};
        kw.nparts = tt.lane_parts;
        for (int pq = 0; pq < FBR_KINWRITE_PARTS; pq++) {
            kw.part_nsteps[pq] = tt.lane_nsteps[pq];
            kw.part_step0[pq] = tt.lane_step0[pq];
        }
        kw.lcol10 = t + tt.o_lcol;
        kw.colrec = t + tt.o_lrec;
        kw.dst = (const long *)(c.dtab + c.o_lent) + (size_t)set * c.nlent;
        kw.ninert = hm.ninert;
        kw.cols = hm.cols;
        kw.k = k;
        kw.has_w = dw ? 1 : 0;
        const size_t lane_lds = tt.lane_lds;
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8 / tt.lane_parts, (size_t)(150 << 10) / std::max<size_t>(lane_lds, 1)));
        const int blocks = (int)std::min<long>((cs + 63) / 64, (long)m->num_cus * per_cu);
        if ((rc = m->kinid_scratch.ensure((size_t)blocks * tt.lane_parts * std::max(kp.nslots, 1) * FBR_LINK_REC * 64 * sizeof(double)))) return rc;
        ProfScope ps(m, FBR_PROF_REGRESSOR, cst);
        if ((rc = fbr_by_depth<4, 8, 10, 12, FBR_KINID_MAXD>(kp.maxlvl, [&](auto D) -> int {
                 HIPCHK(hipFuncSetAttribute((const void *)fbr_kinwrite_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lane_lds));
                 hipLaunchKernelGGL(fbr_kinwrite_kernel<D>, dim3(blocks), dim3(64 * tt.lane_parts), lane_lds, cst, m->dm, kp, kw, cs, d.q + s0 * hm.n,
                                    d.dq + s0 * hm.n, d.ddq + s0 * hm.n, d.bv ? d.bv + s0 * 6 : nullptr, d.ba ? d.ba + s0 * 6 : nullptr,
                                    d.rpy ? d.rpy + s0 * 3 : nullptr, d.sign ? d.sign + s0 * hm.n : nullptr,
                                    drhs ? drhs + (size_t)s0 * hm.rows * k : nullptr, dw ? dw + (size_t)s0 * hm.rows : nullptr,
                                    m->kinid_scratch.as<double>());
                 return FBR_OK;
             })))
            return rc;
    } else {
        // the kinematic records are produced for several chunks at a time: one lane per sample needs tens of thousands of waves in flight
        // to hide its latencies (1 M samples: 6.4 ms in one launch, 11 ms in twelve)
        const long kin_span = std::max(ch, std::min(S, (long)((size_t)(6ull << 30) / ((size_t)hm.rec_size() * sizeof(double))) / ch * ch));
        const long k0 = s0 / kin_span * kin_span;
        if (s0 == k0 && (rc = run_kin(m, d, k0, std::min(kin_span, S - k0), cst))) return rc;
        const double *recs = m->rec.as<double>() + (size_t)(s0 - k0) * hm.rec_size();
        if (csp > cs) {
            hipLaunchKernelGGL(fbr_groups_clear_pad_kernel, dim3(G, (unsigned)maxrows), dim3(256), 0, cst, c.dgrp, t + tt.o_nrows, cs, csp);
            HIPCHK(hipGetLastError());
        }
        // (the writers take the entry lists of variant 1: the structural zeros left of a row's first supported column tile are never written)
        const unsigned grid = (unsigned)std::min<long>(cs, (long)m->num_cus * 8);
        const double *dq = d.dq + s0 * hm.n, *sign = d.sign ? d.sign + s0 * hm.n : nullptr;
        const double *rhs = drhs ? drhs + (size_t)s0 * hm.rows * k : nullptr, *w = dw ? dw + (size_t)s0 * hm.rows : nullptr;
        const int *ents = (const int *)(c.dtab + c.o_ent1);
        ProfScope ps(m, FBR_PROF_REGRESSOR, cst);
        if (c.lds_writer)
            hipLaunchKernelGGL(fbr_regressor_groups_lds_kernel, dim3(grid), dim3(256), c.lds_img, cst, m->dm, cs, recs, dq, sign, rhs, k, w, c.dgrp, G, t,
                               t + hm.rows, t + tt.o_ebeg[1], ents, t + tt.o_rowoff, c.img_total, csp, (int)tt.ents[1].size());
        else if (tt.pairable)
            hipLaunchKernelGGL(fbr_regressor_groups2_kernel, dim3(grid), dim3(256), c.lds, cst, m->dm, cs, recs, dq, sign, rhs, k, w, c.dgrp, G, t,
                               t + hm.rows, t + tt.o_ebeg[1], ents, t + tt.o_pbeg[1], (const int *)(c.dtab + c.o_pent1), tt.npairs, hm.ninert,
                               tt.wsplit, csp);
        else
            hipLaunchKernelGGL(fbr_regressor_groups_kernel, dim3(grid), dim3(256), c.lds, cst, m->dm, cs, recs, dq, sign, rhs, k, w, c.dgrp, G, t,
                               t + hm.rows, t + tt.o_ebeg[1], ents, csp);
    }
    HIPCHK(hipGetLastError());
    return FBR_OK;
}

// level-0 fold of group g's chunk (csp rows per slot) on the main stream
static int tsqr_fold_group(TsqrGroupCall &c, int g, long csp)
{
    const TsqrGroup &Gg = c.gp.groups[g];
    FbrTsqrRowOrder ro;
    ro.first_col = c.t + c.tt.o_fc[g];
    ro.rows = (int)Gg.rows.size();
    ro.group = csp;
    if (c.tt.lane_writer) ro.colmajor_ld = csp * (long)Gg.rows.size();
    if (int rc = fbr_tsqr_fold_chunk(c.work(g), c.m->stream, csp * (long)Gg.rows.size(), Gg.Pa, 0, nullptr, ro)) return tsqr_status(rc, "tsqr group fold");
    return FBR_OK;
}

// The side groups' merge trees, on the side streams behind what the main stream has enqueued; tsqr_ev[i] marks the end of side stream i
static int tsqr_side_trees(TsqrGroupCall &c)
{
    fbr_model *m = c.m;
    HIPCHK(hipEventRecord(m->tsqr_ev[TSQR_NSIDE], m->stream));
    for (int i = 0; i < TSQR_NSIDE; i++) HIPCHK(hipStreamWaitEvent(m->tsqr_streams[i], m->tsqr_ev[TSQR_NSIDE], 0));
    // (narrow factors of one shape -- the two arms, the two legs -- share their launches: fbr_tsqr_finish_narrow_batch)
    int nside = 0, rc;
    std::vector<char> finished(c.gp.groups.size(), 0);
    for (int g : c.side_order) {
        if (finished[g]) continue;
        FbrTsqrWork &wg = m->tsqr_groups[g];
        FbrTsqrWork *batch[FBR_TSQR_NARROW_BATCH];
        double *outs[FBR_TSQR_NARROW_BATCH];
        int nb = 0;
        if (wg.narrow)
            for (int h : c.side_order)
                if (!finished[h] && nb < FBR_TSQR_NARROW_BATCH && m->tsqr_groups[h].narrow && m->tsqr_groups[h].n == wg.n && m->tsqr_groups[h].NW == wg.NW &&
                    m->tsqr_groups[h].tpw == wg.tpw) {
                    batch[nb] = &m->tsqr_groups[h];
                    outs[nb++] = c.rtmp + c.o_r[h];
                    finished[h] = 1;
                }
        hipStream_t sst = m->tsqr_streams[nside++ % TSQR_NSIDE];
        if (nb >= 2) {
            if ((rc = fbr_tsqr_finish_narrow_batch(batch, nb, sst, outs))) return tsqr_status(rc, "tsqr group finish");
        } else {
            for (int i = 0; i < nb; i++) finished[(int)(batch[i] - &m->tsqr_groups[0])] = 0;  // (a batch of one: the plain path)
            finished[g] = 1;
            if ((rc = fbr_tsqr_finish_async(wg, sst, c.rtmp + c.o_r[g]))) return tsqr_status(rc, "tsqr group finish");
        }
    }
    for (int i = 0; i < TSQR_NSIDE; i++) HIPCHK(hipEventRecord(m->tsqr_ev[i], m->tsqr_streams[i]));
    return FBR_OK;
}

// what a following submission's prologue waits for
static int tsqr_record_l0(fbr_model *m)
{
    HIPCHK(hipEventRecord(m->ev_tsqr_l0, m->stream));
    m->tsqr_l0_rec = true;
    return FBR_OK;
}

// The final factor with a dense main group: the erows stacked rows of the embedded group factors ([sum of the side groups' Pa][n], the
// final factor's column order) are folded into the factors alive inside the main group's tree, which then runs to its end
static int tsqr_final_inside(TsqrGroupCall &c, long erows, double *R)
{
    fbr_model *m = c.m;
    FbrTsqrWork &wk = m->tsqr;
    int rc;
    int alive_stride = 1;  // levels with stride < alive_stride have run
    while ((wk.NW + alive_stride - 1) / alive_stride > 8) alive_stride *= 2;
    // (a following submission's prologue starts behind the two widest tree levels: 128 and 64 workgroups)
    const int s_pro = std::min(4, alive_stride);
    {
        ProfScope ps(m, FBR_PROF_TREE);
        if ((rc = fbr_tsqr_tree_levels(wk, m->stream, 1, s_pro)) || (rc = tsqr_record_l0(m)) || (rc = fbr_tsqr_tree_levels(wk, m->stream, s_pro, alive_stride)))
            return tsqr_status(rc, "tsqr tree");
    }
    for (int i = 0; i < TSQR_NSIDE; i++) HIPCHK(hipStreamWaitEvent(m->stream, m->tsqr_ev[i], 0));
    const long epad = (erows + 15) & ~15L;
    if ((rc = m->tsqr_embed.ensure((size_t)epad * wk.n * sizeof(double)))) return rc;
    double *emb = m->tsqr_embed.as<double>();
    const int alive = (wk.NW + alive_stride - 1) / alive_stride;
    {
        ProfScope ps(m, FBR_PROF_TSQR);
        long off = 0;
        for (size_t i = 0; i < c.side_order.size(); i++) {
            const int g = c.side_order[i], Pg = c.gp.groups[g].Pa;
            const long mp = i + 1 == c.side_order.size() ? epad - off : Pg;  // (the last one also clears the rows up to the padded count)
            hipLaunchKernelGGL(fbr_tsqr_pack_kernel, dim3(256), dim3(256), 0, m->stream, (long)Pg, mp, c.Pa, 0, wk.n, c.rtmp + c.o_r[g], Pg, c.t + c.tt.o_emb[g],
                               (const double *)nullptr, (const double *)nullptr, emb + off * wk.n, 0, 0L);
            HIPCHK(hipGetLastError());
            off += Pg;
        }
        if ((rc = fbr_tsqr_fold_packed(wk, m->stream, erows, FbrTsqrRowOrder(), emb, alive_stride, alive))) return tsqr_status(rc, "tsqr embedded group factors");
    }
    ProfScope ps(m, FBR_PROF_TREE);
    if ((rc = fbr_tsqr_tree_levels(wk, m->stream, alive_stride, 1 << 30)) || (rc = fbr_tsqr_copy_out(wk, m->stream, R))) return tsqr_status(rc, "tsqr tree");
    return FBR_OK;  // (the error word of the call is read once, at its end: tsqr_end_call)
}

// The final factor without a dense group (fixed base behind a branching first link, masked base rows) or with wave-private main
// kernels: one workgroup folds the group factors into a factor seeded with the main group's result / R_in
static int tsqr_final_one_wg(TsqrGroupCall &c, const double *Rin_dev, double *R)
{
    fbr_model *m = c.m;
    const TsqrGroupPlan &gp = c.gp;
    int rc;
    if ((rc = tsqr_record_l0(m))) return rc;
    ProfScope ps(m, FBR_PROF_TSQR);
    const double *seed = Rin_dev;
    if (gp.main >= 0) {
        if ((rc = fbr_tsqr_finish_async(m->tsqr, m->stream, c.rtmp + c.o_r[gp.main]))) return tsqr_status(rc, "tsqr finish");
        seed = c.rtmp + c.o_r[gp.main];
    }
    for (int i = 0; i < TSQR_NSIDE; i++) HIPCHK(hipStreamWaitEvent(m->stream, m->tsqr_ev[i], 0));
    if ((rc = tsqr_begin(m, m->tsqr, m->stream, c.Pa, seed, m->num_cus, 1, m->tsqr_err))) return tsqr_status(rc, "tsqr begin");
    for (int g = 0; g < (int)gp.groups.size(); g++) {
        if (g == gp.main) continue;
        const int Pg = gp.groups[g].Pa;
        if ((rc = fbr_tsqr_fold_rows(m->tsqr, m->stream, Pg, c.Pa, c.rtmp + c.o_r[g], 0, nullptr, nullptr, Pg, c.t + c.tt.o_emb[g])))
            return tsqr_status(rc, "tsqr group merge");
    }
    if ((rc = fbr_tsqr_finish_async(m->tsqr, m->stream, R))) return tsqr_status(rc, "tsqr finish");
    return FBR_OK;
}

// overlap: the call follows a TSQR submission that is still running: its prologue (tables, kinematics and the writer of the first chunk)
// goes to the producer stream and waits only for the LAST LEVEL-0 FOLD of that submission -- it runs beside the submission's merge trees,
// which occupy a handful of CUs (7.7 of WALK-MAN's 8.2 ms of trees hide 5.5 + 1.2 ms of kinematics and first writer).
static int tsqr_groups_impl(fbr_model *m, const DevStates &d, const TsqrGroupPlan &gp, const int32_t *cols, int Psel, int k, const double *drhs,
                            const double *dw, const double *Rin_dev, double *R, int par, bool overlap)
{
    const long S = d.S;
    const int G = (int)gp.groups.size();
    int rc;
    if ((int)m->tsqr_groups.size() < G) m->tsqr_groups.resize(G);
    long lcm = 1;
    const long ch = tsqr_group_chunk_samples(m, gp, S, &lcm);
    if (ch < 0) return tsqr_status(-4, "tsqr group shape");
    TsqrGroupCall c{m, d, gp,
                    tsqr_group_tables(m->hm, gp, cols, Psel, k, dw != nullptr, m->opt.tsqr_writer, m->opt.tsqr_lane_writer != 0, m->kinid.nsteps > 0),
                    drhs, dw, k, Psel + k, ch, lcm};
    if ((rc = ensure_tsqr_streams(m, overlap))) return rc;
    hipStream_t pst = overlap ? m->tsqr_pro_stream : m->stream;
    if ((rc = tsqr_begin_groups(c, Rin_dev, pst, overlap)) || (rc = tsqr_writer_setup(c)) || (rc = tsqr_upload_group_tables(c, par, pst))) return rc;
    // Merge trees are latency bound (a level of the full-width tree is 0.93 ms on a handful of workgroups, 8 levels over 256 private
    // factors).  The groups' trees run on side streams beside the main group's.  Their factors, embedded into the caller's column
    // order, are dense rows of the final factorisation: they are folded INSIDE the main tree -- once at most 8 of its factors are
    // alive, one launch deals the embedded rows to those factors (a block or two per workgroup) -- instead of by one workgroup, group
    // after group, behind the tree (round 3: 3.3 ms per call).  Without a dense group the final factor starts from R_in.
    size_t rt = 0;
    c.o_r.assign(G, 0);
    for (int g = 0; g < G; g++) {
        c.o_r[g] = rt;
        rt += (size_t)gp.groups[g].Pa * gp.groups[g].Pa;
    }
    if ((rc = m->tsqr_rtmp.ensure(rt * sizeof(double)))) return rc;
    c.rtmp = m->tsqr_rtmp.as<double>();
    // the longest trees first, one stream each as far as they go (a short tree queued behind the waist chain's tree was the last to finish)
    for (int g = 0; g < G; g++)
        if (g != gp.main) c.side_order.push_back(g);
    std::stable_sort(c.side_order.begin(), c.side_order.end(), [&](int a, int b) { return gp.groups[a].Pa > gp.groups[b].Pa; });
    // The side groups' trees are started as soon as their last level-0 fold has been enqueued -- BEFORE the main (base-wrench) group's last
    // fold: they are latency bound (eleven levels over 2048 wave-private factors, a handful of waves each at the end: 1.9 ms for the waist
    // chain's group of a 125 k-sample call) and then run beside the throughput-bound fold of the main group instead of behind it.
    bool side_trees_launched = false;
    for (long s0 = 0; s0 < S; s0 += ch) {
        const long cs = std::min(ch, S - s0);
        hipStream_t cst = s0 == 0 ? pst : m->stream;  // the first chunk's kinematics and writer belong to the prologue
        // every slot of the chunk holds csp >= cs rows, a whole number of fold blocks in every group (the last chunk is padded with zero
        // rows): a block never straddles two regressor rows, and the structural zeros left of a row's first supported column tile are
        // never written (the folds do not read them)
        const long csp = (cs + lcm - 1) / lcm * lcm;
        if ((rc = tsqr_write_chunk(c, s0, cs, csp, cst))) return rc;
        if (cst != m->stream) {  // the folds (main stream) wait for the prologue
            HIPCHK(hipEventRecord(m->ev_tsqr_pro, cst));
            HIPCHK(hipStreamWaitEvent(m->stream, m->ev_tsqr_pro, 0));
        }
        ProfScope ps(m, FBR_PROF_TSQR);
        for (int g = 0; g < G; g++)
            if (g != gp.main && (rc = tsqr_fold_group(c, g, csp))) return rc;
        // (last chunk: option tsqr_side_trees_beside = 1 starts the side groups' trees beside the main group's fold.  That paid while the main
        // group folded all six base-wrench rows; with the force rows in a group of their own its fold is half as long, and the trees' first
        // levels only keep its workgroups off their CUs: 125 k samples 7.3 ... 7.45 ms beside, 6.9 ... 7.0 behind; 1 M samples the same)
        if (s0 + ch >= S && gp.main >= 0 && m->opt.tsqr_side_trees_beside != 0) {
            if ((rc = tsqr_side_trees(c))) return rc;
            side_trees_launched = true;
        }
        if (gp.main >= 0 && (rc = tsqr_fold_group(c, gp.main, csp))) return rc;
    }
    if (!side_trees_launched && (rc = tsqr_side_trees(c))) return rc;
    long erows = 0;
    for (int g : c.side_order) erows += gp.groups[g].Pa;
    if (gp.main >= 0 && !m->tsqr.narrow && erows > 0) return tsqr_final_inside(c, erows, R);
    return tsqr_final_one_wg(c, Rin_dev, R);
}

// why a column subset cannot be factorised, or nullptr
static const char *tsqr_cols_problem(const FbrHostModel &hm, const int32_t *cols, int32_t ncols)
{
    if (ncols <= 0 || ncols > hm.cols) return "bad column subset size";
    std::vector<char> seen(hm.cols, 0);
    for (int i = 0; i < ncols; i++) {
        if (cols[i] < 0 || cols[i] >= hm.cols || seen[cols[i]]) return "column subset entries must be distinct and in range";
        seen[cols[i]] = 1;
    }
    return nullptr;
}

// A column subset goes through the reductions (`which`: pick_tsqr_reduction) when it is about as wide as the regrouped column set (the
// base columns: one per direction the regressor can move in) -- a narrow subset is cheaper factorised directly -- and only through the
// regrouped model.  (Invalid lists are reported by the direct path.)
static bool tsqr_subset_via_red(const fbr_model *m, int which, const int32_t *cols, int32_t ncols)
{
    return which == 1 && 5L * ncols >= 4L * m->rdm[1]->hm.cols && !tsqr_cols_problem(m->hm, cols, ncols);
}

// Where a call computes its factor: R_out, or for a host output the device buffer g_tmp; *Rin_dev: R_in on the device (a host R_in is
// copied into that buffer, which the factorisation is then seeded from)
static int tsqr_stage_output(fbr_model *m, const double *R_in, double *R_out, int32_t out_mem, size_t count, double **R, const double **Rin_dev)
{
    *R = R_out;
    *Rin_dev = R_in;
    if (out_mem == FBR_HOST) {
        if (int rc = m->g_tmp.ensure(count * sizeof(double))) return rc;
        *R = m->g_tmp.as<double>();
        if (R_in) {
            HIPCHK(hipMemcpyAsync(*R, R_in, count * sizeof(double), hipMemcpyHostToDevice, m->stream));
            *Rin_dev = *R;
        }
    }
    return FBR_OK;
}

// The end of every call: the call's error word goes to the pinned slot of its parity; a submission returns its ticket (via_red: 1 + the
// reduced model the pass ran on, red_ticket: that model's ticket), a blocking call waits and looks at the slot
static int tsqr_end_call(fbr_model *m, int par, int64_t *async_ticket, double *R, double *R_out, size_t count, int32_t out_mem, int via_red = 0,
                         int64_t red_ticket = -1)
{
    HIPCHK(hipMemcpyAsync(&m->tsqr_err_host[par], m->tsqr_err, sizeof(unsigned), hipMemcpyDeviceToHost, m->stream));
    if (async_ticket) {
        const int64_t t = m->next_ticket++;
        m->ticket_kind[t & 1] = 1;
        if (via_red) {
            m->ticket_via_red[t & 1] = via_red;
            m->red_ticket[t & 1] = red_ticket;
        }
        m->last_submit_kind = 1;
        HIPCHK(hipEventRecord(m->ev_done[t & 1], m->stream));
        *async_ticket = t;
        return FBR_OK;
    }
    if (int rc = finish_output(m, R, R_out, count, out_mem)) return rc;
    if (m->tsqr_err_host[par]) {
        char hx[16];
        snprintf(hx, sizeof hx, "%08x", m->tsqr_err_host[par]);
        m->tsqr_err_host[par] = 0;
        set_err("TSQR pipeline flag wait timed out (internal error, code " + std::string(hx) + ")");
        return FBR_E_HIP;
    }
    return FBR_OK;
}

// async_ticket != nullptr: the factorisation is enqueued and NOT waited for (fbr_tsqr_submit): device-resident inputs and output only.
static int tsqr_impl_inner(fbr_model *m, const fbr_states *st, const int32_t *cols, int32_t ncols, const double *rhs, int32_t k,
                           const double *w, const double *R_in, double *R_out, int32_t out_mem, int64_t *async_ticket)
{
    const bool async = async_ticket != nullptr;
    if (async && (!st || st->mem != FBR_DEVICE || out_mem != FBR_DEVICE)) {
        set_err("fbr_tsqr_submit takes device-resident states, rhs, weights, R_in and R_out");
        return FBR_E_INVALID;
    }
    DevStates d;
    if (m) m->submitting = async;
    int rc = stage_states(m, st, &d);
    if (m) m->submitting = false;
    if (rc) return rc;
    bool overlap = false;
    if (async) {
        // at most two submissions in flight (two sets of tables / error slots / completion events)
        if ((rc = wait_ticket(m, m->next_ticket - 2))) return rc;
        overlap = m->waited_ticket < m->next_ticket - 1 && m->last_submit_kind == 1 && m->tsqr_l0_rec && m->opt.tsqr_prologue_overlap != 0;
    }
    const int par = (int)(m->next_ticket & 1);  // (blocking calls: nothing is in flight, either set is free)
    HIPCHK(hipMemsetAsync(m->tsqr_err, 0, sizeof(unsigned), m->stream));
    if (!R_out || k < 0 || k > FBR_MAX_RHS || (k > 0 && !rhs)) {
        set_err("bad rhs / R_out arguments");
        return FBR_E_INVALID;
    }
    const FbrHostModel &hm = m->hm;
    if (const char *why = cols ? tsqr_cols_problem(hm, cols, ncols) : nullptr) {
        set_err(why);
        return FBR_E_INVALID;
    }
    const long S = d.S;
    const TsqrPlan plan = tsqr_plan(hm, cols, ncols, k, S, m->opt.tsqr_reorder != 0, 16 * FBR_TSQR_NARROW_MAX_TILES);
    const int Psel = plan.Psel, Pa = plan.Pa;
    const size_t rcount = (size_t)Pa * Pa;
    const double *drhs = nullptr, *dw = nullptr;
    if ((rc = stage_one(m, m->st_aux, rhs, (size_t)S * hm.rows * k, st->mem, &drhs))) return rc;
    if ((rc = stage_one(m, m->st_aux2, w, (size_t)S * hm.rows, st->mem, &dw))) return rc;
    double *R = nullptr;
    const double *Rin_dev = nullptr;
    if ((rc = tsqr_stage_output(m, R_in, R_out, out_mem, rcount, &R, &Rin_dev))) return rc;
    {
        // (row weights on the device are scanned for switched-off rows: that read-back waits for the stream, i.e. for a submission in flight)
        std::vector<char> act;
        if ((rc = active_rows(m, dw, S, &act))) return rc;
        const TsqrGroupPlan gp = tsqr_group_plan(hm, cols, ncols, k, &act, m->opt.tsqr_force_group != 0);
        if (hm.rows <= 255 && tsqr_use_groups(m, gp, S)) {  // (the writer's entries hold the regressor row in 8 bits)
            if ((rc = tsqr_groups_impl(m, d, gp, cols, Psel, k, drhs, dw, Rin_dev, R, par, overlap))) return rc;
            return tsqr_end_call(m, par, async_ticket, R, R_out, rcount, out_mem);
        }
    }
    if (hm.masked) return FBR_E_NOT_GROUPED;  // (internal models with column masks factorise by row groups only: the caller takes the merged model)
    // device tables: [fcols (Psel) | perm (Pa) | inv (Pa) | linkpos (L) | row first columns (rows)]
    const int *dcols = nullptr, *dperm = nullptr, *dinv = nullptr, *dlinkpos = nullptr, *dfc = nullptr;
    {
        std::vector<int> tab;
        tab.insert(tab.end(), plan.fcols.begin(), plan.fcols.end());
        tab.insert(tab.end(), plan.perm.begin(), plan.perm.end());
        tab.insert(tab.end(), plan.inv.begin(), plan.inv.end());
        tab.insert(tab.end(), plan.linkpos.begin(), plan.linkpos.end());
        tab.insert(tab.end(), plan.fc.begin(), plan.fc.end());
        const char *dtab = nullptr;
        if ((rc = tsqr_upload_tables(m, par, {{tab.data(), tab.size() * sizeof(int)}}, {0}, tab.size() * sizeof(int), m->stream, &dtab))) return rc;
        const int *t = (const int *)dtab;
        if (cols || (plan.reorder)) dcols = t;  // gather list of the materialised path
        dperm = t + Psel;
        dinv = dperm + Pa;
        if (!cols && plan.reorder) dlinkpos = dinv + Pa;
        dfc = dinv + Pa + plan.linkpos.size();
    }
    // an existing factor seeds working factor 0 directly when the column order is the caller's; in the internal order its rows are
    // folded in like data rows (column gather)
    if ((rc = tsqr_begin(m, m->tsqr, m->stream, Pa, plan.reorder ? nullptr : Rin_dev, m->num_cus, S * (long)hm.rows, m->tsqr_err))) return tsqr_status(rc, "tsqr begin");
    if (plan.reorder && Rin_dev) {
        ProfScope ps(m, FBR_PROF_TSQR);
        if ((rc = fbr_tsqr_fold_rows(m->tsqr, m->stream, Pa, Pa, Rin_dev, 0, nullptr, nullptr, Pa, dperm))) return tsqr_status(rc, "tsqr fold R_in");
    }
    if (S > 0) {
        // materialise Y chunk by chunk (K1 + K2) and fold each chunk into the per-workgroup factors.  Without row
        // weights / column subset the regressor kernel writes straight into the padded chunk [Y | rhs | 0] of the
        // factorisation (leading dimension n): no second pass over Y.
        const size_t per = (size_t)hm.rows * hm.cols;
        long ch = fbr_tsqr_chunk_samples(hm.rows, Pa);
        ch = std::min(ch, chunk_size(m, S));
        if (ch > m->tsqr.mb) ch -= ch % m->tsqr.mb;  // whole blocks per regressor row in the row-sorted chunks
        const bool direct = !cols && !dw;
        if (!direct && (rc = m->out_tmp.ensure((size_t)ch * per * sizeof(double)))) return rc;
        for (long s0 = 0; s0 < S; s0 += ch) {
            const long cs = std::min(ch, S - s0);
            if ((rc = run_kin(m, d, s0, cs))) return rc;
            double *dst = m->out_tmp.as<double>();
            int ldy = hm.cols;
            // The chunk is stacked by regressor row (all samples' row r together): R does not depend on the order of the rows,
            // and a 64-row block of one regressor row is zero left of that row's first supported column, so its fold starts
            // there (rows of joints deep in the tree touch a fraction of the panels).
            FbrTsqrRowOrder ro;
            ro.first_col = dfc;
            ro.rows = hm.rows;
            ro.group = cs;
            long rs_s = hm.rows, rs_r = 1;
            if (direct) {
                if ((rc = fbr_tsqr_chunk_buffer(m->tsqr, cs * hm.rows, &dst)) || (k == 0 && (rc = fbr_tsqr_chunk_clean(m->tsqr, m->stream))))
                    return tsqr_status(rc, "tsqr chunk");
                ldy = m->tsqr.n;
                if (ro.rows) {
                    rs_s = 1;
                    rs_r = cs;
                }
            }
            const int *lp = direct ? dlinkpos : nullptr;  // (the materialised path gathers the columns when it packs the chunk)
            // structural zeros left of a row's first supported column tile are not written when every block holds rows of ONE regressor
            // row (the chunk is a whole number of blocks per row): the folds never read them
            const int *skipfc = (direct && cs % m->tsqr.mb == 0) ? dfc : nullptr;
            if ((rc = launch_regressor(m, d, s0, cs, dst, ldy, rs_s, rs_r, lp, skipfc))) return rc;
            ProfScope ps(m, FBR_PROF_TSQR);
            if (direct)
                rc = fbr_tsqr_fold_chunk(m->tsqr, m->stream, cs * hm.rows, Psel, k, drhs ? drhs + (size_t)s0 * hm.rows * k : nullptr, ro);
            else
                rc = fbr_tsqr_fold_rows(m->tsqr, m->stream, cs * hm.rows, Psel, m->out_tmp.as<double>(), k,
                                        drhs ? drhs + (size_t)s0 * hm.rows * k : nullptr, dw ? dw + (size_t)s0 * hm.rows : nullptr, hm.cols, dcols, ro);
            if (rc) return tsqr_status(rc, "tsqr fold");
        }
    }
    {
        ProfScope ps(m, FBR_PROF_TSQR);
        if (!plan.reorder) {
            if ((rc = fbr_tsqr_finish_async(m->tsqr, m->stream, R))) return tsqr_status(rc, "tsqr finish");
        } else {
            // factor in the internal column order -> the caller's: R = qr(R' [:, inv]) (one workgroup, Pa dense rows)
            if ((rc = m->tsqr_rtmp.ensure(rcount * sizeof(double)))) return rc;
            if ((rc = fbr_tsqr_finish_async(m->tsqr, m->stream, m->tsqr_rtmp.as<double>()))) return tsqr_status(rc, "tsqr finish");
            if ((rc = tsqr_begin(m, m->tsqr, m->stream, Pa, nullptr, m->num_cus, 1, m->tsqr_err)) ||
                (rc = fbr_tsqr_fold_rows(m->tsqr, m->stream, Pa, Pa, m->tsqr_rtmp.as<double>(), 0, nullptr, nullptr, Pa, dinv)) ||
                (rc = fbr_tsqr_finish_async(m->tsqr, m->stream, R)))
                return tsqr_status(rc, "tsqr column order");
        }
    }
    return tsqr_end_call(m, par, async_ticket, R, R_out, rcount, out_mem);
}
// the reduced model a factorisation of every column runs on (-1: the model itself); the regrouped model factorises by row groups only
static int pick_tsqr_reduction(fbr_model *m, long S)
{
    if (!m->opt.link_merge) return -1;
    // (like the Gram pass, pick_gram_reduction: the reduced factorisation costs a second model's launches and one expansion level; a
    // factorisation does about eight times the work of a Gram pass per sample and column pair, hence an eighth of its threshold)
    if (const fbr_model *r0 = m->rdm[0] ? m->rdm[0].get() : m->rdm[1].get();
        r0 && S >= 0 && (double)S * (m->hm.cols - r0->hm.cols) * m->hm.cols < m->opt.reduce_min_work / 8) return -1;
    if (m->rdm[1] && m->opt.regroup && m->opt.tsqr_groups) {
        if (m->rd_grouped < 0) {
            const TsqrGroupPlan gp = tsqr_group_plan(m->rdm[1]->hm, nullptr, 0, 0, nullptr, m->opt.tsqr_force_group != 0);
            m->rd_grouped = gp.groups.size() > 1 && m->rdm[1]->hm.rows <= 255;
        }
        if (m->rd_grouped && S >= (long)m->opt.tsqr_group_min_samples) return 1;
    }
    return m->rdm[0] ? 0 : -1;
}

// The factor through the link-merged model (build_reduction): R_red over the moving bodies' columns, then R = qr([R_in ; R_red E]) --
// the Pra dense rows R_red E become working factor 1 beside R_in (or zero) in working factor 0, and ONE level of the merge tree,
// pipelined across workgroups, folds them (wide factors; narrow ones fold them as ordinary rows).
// cols != NULL: the factor of a COLUMN SUBSET (fbr_tsqr_cols): Y[:, cols] = Y_red E[:, cols], so the reduced factorisation is the same and
// only the expansion takes the subset's columns of E -- the base regressor [YBase | tau] of WALK-MAN (213 of 480 columns, spread over
// every link) costs the regrouped factorisation's 57 ms per 1 M samples instead of 68.
static int tsqr_via_red(fbr_model *m, int which, const fbr_states *st, const int32_t *cols, int32_t ncols, const double *rhs, int32_t k, const double *w,
                        const double *R_in, double *R_out, int32_t out_mem, int64_t *async_ticket)
{
    fbr_model *r = m->rdm[which].get();
    const bool async = async_ticket != nullptr;
    int rc;
    if ((rc = enter(m))) return rc;
    if ((rc = wait_ticket(m, async ? m->next_ticket - 2 : m->next_ticket - 1))) return rc;
    if (async && out_mem != FBR_DEVICE) {
        set_err("fbr_tsqr_submit takes device-resident states, rhs, weights, R_in and R_out");
        return FBR_E_INVALID;
    }
    r->stream = m->stream;
    r->prof = m->prof;
    const int par = (int)(m->next_ticket & 1), Pa = (cols ? ncols : m->hm.cols) + k, Pra = r->hm.cols + k;
    const size_t cnt = (size_t)Pa * Pa;
    if ((rc = m->red_out[par].ensure((size_t)Pra * Pra * sizeof(double)))) return rc;
    double *Rred = m->red_out[par].as<double>();
    int64_t tr = -1;
    if ((rc = tsqr_impl(r, st, nullptr, 0, rhs, k, w, nullptr, Rred, FBR_DEVICE, async ? &tr : nullptr))) return rc;
    const int *dcolmap = nullptr;  // output column jj of the subset -> column of the augmented full layout (rhs columns behind the identified ones)
    if (cols) {
        std::vector<int> cmap(cols, cols + ncols);
        for (int i = 0; i < k; i++) cmap.push_back(m->hm.cols + i);
        const char *dtab = nullptr;
        if ((rc = tsqr_upload_tables(m, par, {{cmap.data(), cmap.size() * sizeof(int)}}, {0}, cmap.size() * sizeof(int), m->stream, &dtab))) return rc;
        dcolmap = (const int *)dtab;
    }
    double *R = nullptr;
    const double *Rin_dev = nullptr;
    if ((rc = tsqr_stage_output(m, R_in, R_out, out_mem, cnt, &R, &Rin_dev))) return rc;
    HIPCHK(hipMemsetAsync(m->tsqr_err, 0, sizeof(unsigned), m->stream));
    FbrTsqrShape sh;
    if (fbr_tsqr_shape(Pa, m->num_cus, 1, &sh, topts(m))) return tsqr_status(-4, "tsqr shape");
    FbrTsqrWork &wk = m->tsqr;
    {
        ProfScope ps(m, FBR_PROF_TREE);
        bool done_wide = false;
        // (the kernels whose merge level takes dense partner rows; a working factor has room for sh.n of them: a column subset narrower
        // than the reduced column set -- Pra > Pa -- takes the row path below)
        if (!sh.narrow && sh.n / 16 > FBR_TSQR_NARROW_MAX_TILES && !m->opt.tsqr_tree_one_wg && Pra <= sh.n) {
            if ((rc = tsqr_begin(m, wk, m->stream, Pa, Rin_dev, m->num_cus, 2L * sh.mb, m->tsqr_err))) return tsqr_status(rc, "tsqr begin");
            if (wk.NW == 2) {
                if ((rc = launch_expand_rows(m, which, k, Pra, Rred, wk.Rw + (size_t)wk.n * wk.ld, wk.ld, dcolmap, Pa))) return rc;
                if ((rc = fbr_tsqr_tree_levels(wk, m->stream, 1, 2, Pra)) || (rc = fbr_tsqr_copy_out(wk, m->stream, R))) return tsqr_status(rc, "tsqr expansion");
                done_wide = true;
            }
        }
        if (!done_wide) {  // narrow factors: the expanded rows as ordinary data rows of a one-workgroup factorisation
            if ((rc = m->tsqr_embed.ensure((size_t)Pra * Pa * sizeof(double)))) return rc;
            if ((rc = launch_expand_rows(m, which, k, Pra, Rred, m->tsqr_embed.as<double>(), Pa, dcolmap, Pa))) return rc;
            if ((rc = tsqr_begin(m, wk, m->stream, Pa, Rin_dev, m->num_cus, 1, m->tsqr_err)) ||
                (rc = fbr_tsqr_fold_rows(wk, m->stream, Pra, Pa, m->tsqr_embed.as<double>(), 0, nullptr, nullptr, Pa)) ||
                (rc = fbr_tsqr_finish_async(wk, m->stream, R)))
                return tsqr_status(rc, "tsqr expansion");
        }
    }
    return tsqr_end_call(m, par, async_ticket, R, R_out, cnt, out_mem, 1 + which, tr);
}

int tsqr_impl(fbr_model *m, const fbr_states *st, const int32_t *cols, int32_t ncols, const double *rhs, int32_t k,
              const double *w, const double *R_in, double *R_out, int32_t out_mem, int64_t *async_ticket)
{
    auto drained = [&](int rc) {  // (blocking calls too: the groups' trees run on side streams)
        if (rc && m && m->pid == getpid() && m->stream) {
            const std::string msg = g_fbr_err;
            drain_after_failed_submit(m);
            set_err(msg);
        }
        return rc;
    };
    int which = (m && st && R_out && k >= 0 && k <= FBR_MAX_RHS && m->pid == getpid()) ? pick_tsqr_reduction(m, (long)st->num_samples) : -1;
    if (cols && which >= 0 && !tsqr_subset_via_red(m, which, cols, ncols)) which = -1;
    while (which >= 0) {
        int rc = tsqr_via_red(m, which, st, cols, ncols, rhs, k, w, R_in, R_out, out_mem, async_ticket);
        if (rc == FBR_E_NOT_GROUPED && which == 1) {  // (row weights left the regrouped model without row groups: see tsqr_impl_inner)
            which = (m->rdm[0] && !cols) ? 0 : -1;
            continue;
        }
        return drained(rc);
    }
    int rc = tsqr_impl_inner(m, st, cols, ncols, rhs, k, w, R_in, R_out, out_mem, async_ticket);
    // FBR_E_NOT_GROUPED (a reduced model with column masks whose row weights left it without row groups) is not a failure: only the
    // clearing of the error word and the staging of rhs / weights were enqueued, nothing that reads the caller's buffers stays in
    // flight, and the caller (tsqr_impl of the parent) repeats the call on the merged model -- no drain: it would serialise an
    // asynchronous submission and mark tickets as waited whose error words have not been looked at
    return rc == FBR_E_NOT_GROUPED ? rc : drained(rc);
}

extern "C" int fbr_tsqr(fbr_model *m, const fbr_states *st, const double *rhs, int32_t k, const double *w,
                        const double *R_in, double *R_out, int32_t out_mem)
{
    return tsqr_impl(m, st, nullptr, 0, rhs, k, w, R_in, R_out, out_mem, nullptr);
}

extern "C" int fbr_tsqr_cols(fbr_model *m, const fbr_states *st, const int32_t *cols, int32_t ncols, const double *rhs,
                             int32_t k, const double *w, const double *R_in, double *R_out, int32_t out_mem)
{
    if (!cols) {
        set_err("cols is NULL");
        return FBR_E_INVALID;
    }
    return tsqr_impl(m, st, cols, ncols, rhs, k, w, R_in, R_out, out_mem, nullptr);
}

extern "C" int fbr_tsqr_submit(fbr_model *m, const fbr_states *st, const int32_t *cols, int32_t ncols, const double *rhs, int32_t k,
                               const double *w, const double *R_in, double *R_out, int64_t *ticket)
{
    if (!ticket) {
        set_err("ticket is NULL");
        return FBR_E_INVALID;
    }
    if (cols && ncols <= 0) {
        set_err("bad column subset size");
        return FBR_E_INVALID;
    }
    return tsqr_impl(m, st, cols, cols ? ncols : 0, rhs, k, w, R_in, R_out, FBR_DEVICE, ticket);
}

// ---- executed MFMA instructions of a factorisation (fbr_tsqr_work_info)
// one fold of a block whose first supported column is first_col: V^T C (4 SUB) + T (4) + C -= V W (4 SUB) per (panel, tile right of it)
static long tsqr_fold_mfma(const FbrTsqrShape &sh, int first_col)
{
    const long np_ = sh.n / 16 - first_col / 16;
    return np_ > 0 ? (8L * sh.sub + 4) * (np_ * (np_ - 1) / 2) : 0;
}
// `rows` dense rows (padded to 16) folded into one working factor, sh.mb rows at a time
static long tsqr_dense_fold_mfma(const FbrTsqrShape &sh, long rows)
{
    long t = 0;
    for (long r0 = 0; r0 < ((rows + 15) & ~15L); r0 += sh.mb) t += tsqr_fold_mfma(sh, 0);
    return t;
}
// one node of a merge tree (a tree over NW working factors has NW - 1): the partner's triangular factor folded in tmb-row pieces
static long tsqr_merge_node_mfma(const FbrTsqrShape &sh)
{
    long t = 0;
    for (int i0 = 0; i0 < sh.n; i0 += sh.tmb) {
        const long np_ = sh.n / 16 - i0 / 16;
        t += np_ > 0 ? (8L * sh.tsub + 4) * (np_ * (np_ - 1) / 2) : 0;
    }
    return t;
}
static long tsqr_tree_mfma(const FbrTsqrShape &sh) { return (sh.NW - 1) * tsqr_merge_node_mfma(sh); }
// the level-0 folds of S samples in chunks of ch, each padded to a multiple of lcm samples per slot and stacked by slot (fc.size() slots,
// slot r supported from column fc[r]): a block is folded from the first supported column of its rows
static long tsqr_level0_mfma(const FbrTsqrShape &sh, const std::vector<int> &fc, long S, long ch, long lcm)
{
    long l0 = 0;
    for (long s0 = 0; s0 < S; s0 += ch) {
        const long cs = (std::min(ch, S - s0) + lcm - 1) / lcm * lcm, M = cs * (long)fc.size(), Mpad = (M + 15) & ~15L;
        for (long r0 = 0; r0 < Mpad; r0 += sh.mb) {
            int f = sh.n;
            if (r0 < M)
                for (long r = r0 / cs; r <= (std::min<long>(r0 + sh.mb, M) - 1) / cs; r++) f = std::min(f, fc[r]);
            l0 += tsqr_fold_mfma(sh, f);
        }
    }
    return l0;
}

extern "C" int fbr_tsqr_work_info(fbr_model *m, const int32_t *cols, int32_t ncols, int32_t k, int64_t num_samples, int64_t *mfma_level0,
                                  int64_t *mfma_tree, int32_t *block_rows, int32_t *n_padded)
{
    if (!m || k < 0 || k > FBR_MAX_RHS || num_samples < 0 || (cols && (ncols <= 0 || ncols > m->hm.cols))) {
        set_err("bad arguments");
        return FBR_E_INVALID;
    }
    if (const char *why = cols ? tsqr_cols_problem(m->hm, cols, ncols) : nullptr) {
        set_err(why);
        return FBR_E_INVALID;
    }
    const long S = (long)num_samples;
    FbrTsqrShape sh;
    auto shape = [&](int P, long rows, FbrTsqrShape *out) { return fbr_tsqr_shape(P, m->num_cus, rows, out, topts(m)) == 0; };
    auto report = [&](long l0, long tr, int mb, int n) {
        if (mfma_level0) *mfma_level0 = l0;
        if (mfma_tree) *mfma_tree = tr;
        if (block_rows) *block_rows = mb;
        if (n_padded) *n_padded = n;
        return FBR_OK;
    };
    long l0 = 0, tr = 0;
    const int which = pick_tsqr_reduction(m, S);
    if (which >= 0 && (!cols || tsqr_subset_via_red(m, which, cols, ncols))) {
        // what fbr_tsqr runs on a link-merged model: the factorisation of the reduced robot, then the Pra expanded rows folded into the
        // final factor by one tree level; block_rows / n_padded describe the FINAL factor (what fbr_tsqr_merge works on)
        if (int rc = fbr_tsqr_work_info(m->rdm[which].get(), nullptr, 0, k, num_samples, &l0, &tr, nullptr, nullptr)) return rc;
        const int Pa = (cols ? ncols : m->hm.cols) + k, Pra = m->rdm[which]->hm.cols + k;
        if (!shape(Pa, 1, &sh)) return tsqr_status(-4, "tsqr shape");
        const long NP = sh.n / 16;
        return report(l0, tr + (Pra + sh.tmb - 1) / sh.tmb * ((8L * sh.tsub + 4) * (NP * (NP - 1) / 2)), sh.mb, sh.n);
    }
    const FbrHostModel &hm = m->hm;
    const TsqrPlan plan = tsqr_plan(hm, cols, ncols, k, S, m->opt.tsqr_reorder != 0, 16 * FBR_TSQR_NARROW_MAX_TILES);
    const int Pa = plan.Pa;
    int mb = 0;
    const TsqrGroupPlan gp = tsqr_group_plan(hm, cols, ncols, k, nullptr, m->opt.tsqr_force_group != 0);
    if (hm.rows <= 255 && tsqr_use_groups(m, gp, S)) {
        // tree-structured path (tsqr_groups_impl): level 0 of every group over its own chunks, the groups' trees, and the final factor
        // that folds the embedded group factors (dense rows) and runs its own tree
        long lcm = 1, mrows = 0, erows = 0;
        const long ch = tsqr_group_chunk_samples(m, gp, S, &lcm);
        if (ch < 0) return tsqr_status(-4, "tsqr shape");
        for (int g = 0; g < (int)gp.groups.size(); g++) {
            mrows += g == gp.main ? S * (long)gp.groups[g].rows.size() : gp.groups[g].Pa;
            erows += g == gp.main ? 0 : gp.groups[g].Pa;
        }
        for (int g = 0; g < (int)gp.groups.size(); g++) {
            const TsqrGroup &G = gp.groups[g];
            if (!shape(G.Pa, g == gp.main ? mrows : S * (long)G.rows.size(), &sh)) return tsqr_status(-4, "tsqr shape");
            l0 += tsqr_level0_mfma(sh, G.fc, S, ch, lcm);
            if (g != gp.main) tr += tsqr_tree_mfma(sh);
        }
        if (!shape(Pa, mrows, &sh)) return tsqr_status(-4, "tsqr shape");
        mb = sh.mb;
        if (gp.main >= 0) tr += tsqr_tree_mfma(sh);  // the dense group's own tree
        if (gp.main >= 0 && !sh.narrow && erows > 0) {
            tr += tsqr_dense_fold_mfma(sh, erows);  // the stacked embedded group factors, folded into the factors alive inside the main tree
        } else {
            if (!shape(Pa, 1, &sh)) return tsqr_status(-4, "tsqr shape");  // (that factorisation is begun for a handful of rows: tsqr_begin(m, .., 1))
            for (int g = 0; g < (int)gp.groups.size(); g++)
                if (g != gp.main) tr += tsqr_dense_fold_mfma(sh, gp.groups[g].Pa);
        }
    } else {
        if (!shape(Pa, S * (long)hm.rows, &sh)) return tsqr_status(-4, "tsqr shape");
        mb = sh.mb;
        if (S > 0) {
            long ch = std::min(fbr_tsqr_chunk_samples(hm.rows, Pa), chunk_size(m, S));
            if (ch > sh.mb) ch -= ch % sh.mb;
            l0 = tsqr_level0_mfma(sh, plan.fc, S, ch, 1);
        }
        tr = tsqr_tree_mfma(sh);
        if (plan.reorder) {  // the factor is brought back to the caller's column order: Pa dense rows folded by one workgroup
            FbrTsqrShape s1;
            if (!shape(Pa, 1, &s1)) return tsqr_status(-4, "tsqr shape");
            tr += tsqr_dense_fold_mfma(s1, Pa);
        }
    }
    return report(l0, tr, mb, sh.n);
}

extern "C" int fbr_tsqr_merge(fbr_model *m, int32_t n, const double *R_a, const double *R_b, double *R_out, int32_t mem)
{
    if (!m || n <= 0 || !R_a || !R_b || !R_out) {
        set_err("bad arguments");
        return FBR_E_INVALID;
    }
    if (int rc_enter = enter_blocking(m)) return rc_enter;
    const size_t cnt = (size_t)n * n;
    int rc;
    const double *da = nullptr, *db = nullptr;
    if ((rc = stage_one(m, m->st_aux, R_a, cnt, mem, &da))) return rc;
    if ((rc = stage_one(m, m->st_aux2, R_b, cnt, mem, &db))) return rc;
    double *R = R_out;
    if (mem == FBR_HOST) {
        if ((rc = m->g_tmp.ensure(cnt * sizeof(double)))) return rc;
        R = m->g_tmp.as<double>();
    }
    // one workgroup (narrow factors: one wave) folds the partner's factor, 64 (32) rows at a time, into a working factor seeded with
    // R_a; a block of the triangular R_b is folded from its first non-zero column.  (rows_hint = 1: a single working factor, no tree.)
    // Wide factors: the two triangles become working factors 0 and 1 and ONE level of the merge tree joins them -- pipelined across up to
    // eight workgroups (fbr_tsqr_tree_x_kernel: 0.33 instead of 0.93 ms for WALK-MAN's 496 columns; the same blocks in the same order,
    // bit-identical).  This is the step on the critical path of the TSQR rank tree across GPUs (flobaroid_amd/dist.py: one merge per level).
    FbrTsqrShape sh;
    if (!fbr_tsqr_shape(n, m->num_cus, 1, &sh, topts(m)) && !sh.narrow && sh.n / 16 > FBR_TSQR_NARROW_MAX_TILES && !m->opt.tsqr_tree_one_wg) {
        FbrTsqrWork &wk = m->tsqr;
        if ((rc = tsqr_begin(m, wk, m->stream, n, da, m->num_cus, 2L * sh.mb))) return tsqr_status(rc, "tsqr merge");  // rows for two blocks: two working factors
        if (wk.NW == 2) {
            hipLaunchKernelGGL(fbr_tsqr_copy_kernel, dim3(256), dim3(256), 0, m->stream, n, db, n, wk.Rw + (size_t)wk.n * wk.ld, wk.ld, wk.n, wk.ld);
            HIPCHK(hipGetLastError());
            if ((rc = fbr_tsqr_finish(wk, m->stream, R))) return tsqr_status(rc, "tsqr merge");
            return finish_output(m, R, R_out, cnt, mem);
        }
    }
    FbrTsqrRowOrder tri;
    tri.rows = -1;
    if ((rc = tsqr_begin(m, m->tsqr, m->stream, n, da, m->num_cus, 1)) ||
        (rc = fbr_tsqr_fold_rows(m->tsqr, m->stream, n, n, db, 0, nullptr, nullptr, 0, nullptr, tri)) ||
        (rc = fbr_tsqr_finish(m->tsqr, m->stream, R)))
        return tsqr_status(rc, "tsqr merge");
    return finish_output(m, R, R_out, cnt, mem);
}
