// fbr_kinid.h -- kinematics + inverse dynamics / prediction FUSED, one lane per sample, the link records never leave the registers.
//
// Replaces the pair fbr_kin_kernel (one lane per sample, 9.5 KB of records written per WALK-MAN sample in partially filled lines) +
// fbr_id_kernel (one wave per sample, the records read back) on the calls that need torques only: fbr_predict (A9, identifier.py:135-141),
// fbr_inverse_dynamics_batch (A3, identification/model.py:239-331, and the simulated base wrench of every floating-base pass,
// model.py:398-413).  The round-5 review priced the pair at 18.9 KB per sample staged through HBM for 1.1 KB of algorithmic I/O.
//
// Formulation (base-frame composite): with F_l = W_l pi_l the wrench of link l in frame A and S_d the motion vector of
// joint d in A,   base rows = sum_l F_l,   tau_d = S_d . sum_{l below d} F_l.   The links are walked parents first (FbrHostModel::order,
// a depth-first order); every lane carries
//   * the record of the link before (the parent of a chain's next link) in registers,
//   * a STACK of the ancestor joints' motion vectors and torque accumulators, indexed by the joint's depth on the path (<= MAXD levels):
//     F_l is added to every ancestor's accumulator when it is formed; a level is written out when another joint takes it,
//   * the records of branch points (links with a child that is not walked right after them) in a per-wave scratch, lanes interleaved
//     (512-byte coalesced lines; 2 records per WALK-MAN sample).
// All lanes of a wave walk the same link at the same time, so every index into the stacks is wave-uniform: the stacks live in
// registers behind scalar branches, never in scratch memory.  The states of a wave's 64 samples are staged through the LDS with
// coalesced loads (a lane reading q[s][d] straight from the row-major arrays touches 64 lines per instruction: 16 x the bytes).
//
// The program (steps, flush lists, slots) is built on the host by fbr_kinid_build -- HIP-free, so that tests/emul runs the same
// program and the same lane body (fbr_kinid_lane) on the CPU (checked there against the CPU restatement of the reference).
#pragma once
#include <type_traits>
#include <vector>

#include "fbr_math.h"
#include "fbr_program.h"

#define FBR_KINID_STEP 8  // ints per step: link, psrc, psave, jtype, dof, level, depth, flushdof
#define FBR_KINID_MAXD 24 // deepest joint path the register-stack instances cover (deeper trees keep the two-kernel path)

#define FBR_KINWRITE_PARTS 4  // waves of a lane-WRITER workgroup = parts the tree is cut into (fbr_kinid_build_parts)

// per-sample record of the suspended base (fbr_kinsusp_kernel -> fbr_susp_scan_kernel), everything in the attachment link's axes about its
// origin O: composite inertia I (xx xy xz yy yz zz), Coriolis coupling B (3 x 3, row-major), joint-motion moment c0, first mass moment mc,
// the base link's pose R (3 x 3) | p and twist [lin; ang] relative to the attachment frame.  Sample-major: the scan reads one record per step.
#define FBR_SUSP_REC 39
#define FBR_SUSP_I 0
#define FBR_SUSP_B 6
#define FBR_SUSP_C0 15
#define FBR_SUSP_MC 18
#define FBR_SUSP_R 21
#define FBR_SUSP_P 30
#define FBR_SUSP_V 33

// (host) the register-stack instance of a lane kernel for a program of depth maxlvl: f(std::integral_constant<int, D>()) with the first
// of the instance depths D... that is >= maxlvl, or the last one
template <int D, int... Ds, class F> inline auto fbr_by_depth(int maxlvl, F &&f)
{
    if constexpr (sizeof...(Ds) > 0)
        if (maxlvl > D) return fbr_by_depth<Ds...>(maxlvl, f);
    return f(std::integral_constant<int, D>());
}

#if defined(__HIPCC__)
// tables every lane of a wave reads at the same index: through the constant address space they are scalar loads
typedef const __attribute__((address_space(4))) long *fbr_clong_ptr;
typedef const __attribute__((address_space(4))) int *fbr_cint_ptr;
typedef const __attribute__((address_space(4))) double *fbr_cdouble_ptr;
#endif

struct FbrKinIdProgram {
    int nsteps = 0, maxlvl = 0, nslots = 0;
    std::vector<int> steps;     // [nsteps][FBR_KINID_STEP]
    std::vector<int> endflush;  // [maxlvl] dof left on level v after the last link (-1: none)
};

// psrc: -1 base link; 0 the parent is the link of the step before (its record is in registers); 1 + b: the parent's record is in slot b.
// psave: slot this link's record is saved to (a later link that is not the next step has it as parent), or -1.
// level: 0-based depth of the link's own joint on its path (-1: fixed joint / base); depth: joints on the link's path (own one included).
// flushdof: the dof that held `level` until now and is complete (every link below it has been walked), or -1.
// keep (optional, [L]): the program walks these links only -- a set closed under parents (fbr_kinid_build_parts).
static inline void fbr_kinid_build(const FbrHostModel &hm, FbrKinIdProgram &p, const std::vector<char> *keep = nullptr)
{
    std::vector<int> ord;
    for (int l : hm.order)
        if (!keep || (*keep)[l]) ord.push_back(l);
    const int L = (int)ord.size();
    p.nsteps = L;
    p.steps.assign((size_t)std::max(L, 1) * FBR_KINID_STEP, -1);
    std::vector<int> lastchild(hm.L, -1);  // the last step whose parent the link is
    for (int k = 0; k < L; k++) {
        const int par = hm.parent[ord[k]];
        if (par >= 0) lastchild[par] = std::max(lastchild[par], k);
    }
    // slots: a link holds one from its own step to the step of its last child whenever that child is not the very next step
    std::vector<int> slot(hm.L, -1), holder;  // holder[b]: link that holds slot b, or -1
    int maxlvl = 0;
    std::vector<int> lvldof(std::max(hm.maxdepth, 1), -1);
    for (int k = 0; k < L; k++) {
        const int l = ord[k], par = hm.parent[l];
        int *st = &p.steps[(size_t)k * FBR_KINID_STEP];
        for (int &h : holder)
            if (h >= 0 && lastchild[h] < k) h = -1;  // (its last child has been walked)
        st[0] = l;
        st[1] = par < 0 ? -1 : (k > 0 && ord[k - 1] == par ? 0 : 1 + slot[par]);
        if (par >= 0 && st[1] != 0 && (slot[par] < 0 || holder[slot[par]] != par)) throw std::runtime_error("fbr_kinid_build: parent record not held");
        st[2] = -1;
        if (lastchild[l] > k + 1) {  // some child comes later than the next step
            int b = 0;
            while (b < (int)holder.size() && holder[b] >= 0) b++;
            if (b == (int)holder.size()) holder.push_back(-1);
            holder[b] = l;
            slot[l] = st[2] = b;
        }
        st[3] = hm.jtype[l];
        st[4] = hm.dof[l];
        const int depth = (int)hm.path[l].size();
        st[5] = (par >= 0 && hm.dof[l] >= 0) ? depth - 1 : -1;
        st[6] = depth;
        st[7] = -1;
        if (st[5] >= 0) {
            // the joint that held this level is complete: every link below it has been walked (a link adds to level v only if its
            // path has more than v joints, i.e. passes through the joint that holds level v at that moment)
            st[7] = lvldof[st[5]];
            lvldof[st[5]] = hm.dof[l];
            maxlvl = std::max(maxlvl, st[5] + 1);
        }
    }
    const int nslots = (int)holder.size();
    p.nslots = nslots;
    p.maxlvl = maxlvl;
    p.endflush.assign(std::max(maxlvl, 1), -1);
    for (int v = 0; v < maxlvl; v++) p.endflush[v] = lvldof[v];
}

// The tree cut into `nparts` programs for waves that share one block of samples (the lane writer: every wave walks ITS links and the
// ancestors they need, and writes the columns of its own links only).  The depth-first order is cut into contiguous ranges of about
// equal cost (cost[l]: what link l costs its owner); own[p][l] = 1: part p owns link l.  Ancestors are walked redundantly (a trunk of a
// few links on WALK-MAN); nothing is exchanged between the waves.
static inline void fbr_kinid_build_parts(const FbrHostModel &hm, const std::vector<double> &cost, int nparts, std::vector<FbrKinIdProgram> &progs,
                                         std::vector<std::vector<char>> &own)
{
    nparts = std::max(1, std::min(nparts, hm.L));
    double total = 0.0;
    for (int l = 0; l < hm.L; l++) total += cost[l];
    progs.assign(nparts, FbrKinIdProgram());
    own.assign(nparts, std::vector<char>(hm.L, 0));
    double acc = 0.0;
    int part = 0;
    for (int k = 0; k < hm.L; k++) {
        const int l = hm.order[k];
        // (a part is closed when its share is reached; the last part takes what is left; every part gets at least one link)
        if (part + 1 < nparts && acc >= total * (part + 1) / nparts && hm.L - k >= nparts - part - 1) part++;
        own[part][l] = 1;
        acc += cost[l];
    }
    for (int p = 0; p < nparts; p++) {
        std::vector<char> keep = own[p];
        for (int l = 0; l < hm.L; l++)
            if (own[p][l])
                for (int a = hm.parent[l]; a >= 0 && !keep[a]; a = hm.parent[a]) keep[a] = 1;
        fbr_kinid_build(hm, progs[p], &keep);
    }
}

// The same parts from given cut points: part p owns positions [starts[p], starts[p + 1]) of the depth-first order (starts: nparts + 1
// non-decreasing positions from 0 to L; an empty part walks nothing).
static inline void fbr_kinid_build_parts_at(const FbrHostModel &hm, const std::vector<int> &starts, std::vector<FbrKinIdProgram> &progs,
                                            std::vector<std::vector<char>> &own)
{
    const int nparts = (int)starts.size() - 1;
    if (nparts < 1 || starts[0] != 0 || starts[nparts] != hm.L) throw std::runtime_error("fbr_kinid_build_parts_at: cut points outside the order");
    progs.assign(nparts, FbrKinIdProgram());
    own.assign(nparts, std::vector<char>(hm.L, 0));
    for (int p = 0; p < nparts; p++) {
        if (starts[p + 1] < starts[p]) throw std::runtime_error("fbr_kinid_build_parts_at: cut points out of order");
        for (int k = starts[p]; k < starts[p + 1]; k++) own[p][hm.order[k]] = 1;
        std::vector<char> keep = own[p];
        for (int l = 0; l < hm.L; l++)
            if (own[p][l])
                for (int a = hm.parent[l]; a >= 0 && !keep[a]; a = hm.parent[a]) keep[a] = 1;
        fbr_kinid_build(hm, progs[p], &keep);
    }
}
// the cut points of an assignment fbr_kinid_build_parts made (contiguous ranges of the order)
static inline std::vector<int> fbr_kinid_parts_starts(const FbrHostModel &hm, const std::vector<std::vector<char>> &own)
{
    std::vector<int> starts{0};  // (a trailing part may be empty: a dear last link leaves the parts before it short of their share)
    for (size_t p = 0; p < own.size(); p++) {
        int cnt = 0;
        for (int l = 0; l < hm.L; l++) cnt += own[p][l] != 0;
        starts.push_back(starts.back() + cnt);
    }
    return starts;
}

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
#define FBR_UNI(x) __builtin_amdgcn_readfirstlane(x)  // the program is the same for every lane: keep it in scalar registers
#else
#define FBR_UNI(x) (x)
#endif

// ------------------------------------------------------------------------------------------------
// One lane = one sample (or one perturbed evaluation of a sample).  StateFn(d, q, dq, ddq): joint state of dof d; BaseFn(bv6, ba6, rpy3);
// save(b, i, v) / load(b, i): slot b of the branch-point records; ConstFn(l, restR, restp, axis);
// LinkFn(l, depth, rec, Sst, lvd, F): called once per link with its record, the motion vectors Sst[0 .. depth) and dofs lvd[0 .. depth) of
// the joints on its path; with ACC it returns the link's wrench F (frame A), which the lane adds to the base rows and to every ancestor
// joint's torque; Emit(row, value): regressor row `row` of this sample (ACC only; joint rows without friction: the caller adds it).
// `steps` / `endflush` of FbrKinIdProgram; every table access is wave-uniform.
// ------------------------------------------------------------------------------------------------
template <int MAXD, bool ACC, class StateFn, class BaseFn, class SlotSave, class SlotLoad, class LinkFn, class EmitFn, class ConstFn>
FBR_HD void fbr_kinid_lane(int nsteps, int maxlvl, const int *steps, const int *endflush, int floating, const double *g, int fb,
                           StateFn state, BaseFn basest, SlotSave save, SlotLoad load, LinkFn link, EmitFn emit, ConstFn consts)
{
    double P[FBR_LINK_REC];
    double Sst[MAXD][6], tac[MAXD];
    int lvd[MAXD];
    double T[6] = {0, 0, 0, 0, 0, 0};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < MAXD; j++) {
        tac[j] = 0.0;
        lvd[j] = 0;
        for (int i = 0; i < 6; i++) Sst[j][i] = 0.0;
    }
    for (int k = 0; k < nsteps; k++) {
#if defined(__HIP_DEVICE_COMPILE__)
        const fbr_cint_ptr st = (fbr_cint_ptr)(unsigned long)(steps + k * FBR_KINID_STEP);  // (the step program: scalar loads)
#else
        const int *st = steps + k * FBR_KINID_STEP;
#endif
        const int l = FBR_UNI(st[0]), psrc = FBR_UNI(st[1]), psave = FBR_UNI(st[2]), jt = FBR_UNI(st[3]), d = FBR_UNI(st[4]), lvl = FBR_UNI(st[5]),
                  depth = FBR_UNI(st[6]), fd = FBR_UNI(st[7]);
        double out[FBR_LINK_REC], Sv[6] = {0, 0, 0, 0, 0, 0};
        if (psrc < 0) {
            double v6[6] = {0, 0, 0, 0, 0, 0}, a6[6] = {0, 0, 0, 0, 0, 0}, e3[3] = {0, 0, 0};
            if (floating) basest(v6, a6, e3);
            fbr_kin_base(floating, g, v6, a6, e3, out);
        } else {
            if (psrc > 0)
                for (int i = 0; i < FBR_LINK_REC; i++) P[i] = load(psrc - 1, i);
            double rR[9], rp[3], ax[3];
            consts(l, rR, rp, ax);
            double qv = 0, dqv = 0, ddqv = 0;
            if (d >= 0) state(d, qv, dqv, ddqv);
            fbr_kin_child(P, rR, rp, ax, jt, qv, dqv, ddqv, out, Sv);
        }
        if (psave >= 0)
            for (int i = 0; i < FBR_LINK_REC; i++) save(psave, i, out[i]);
        for (int i = 0; i < FBR_LINK_REC; i++) P[i] = out[i];
        // the joint takes its level: whoever held it is complete
        if (lvl >= 0) {
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int j = 0; j < MAXD; j++)
                if (j == lvl) {
                    if (ACC && fd >= 0) emit(fb + fd, tac[j]);
                    tac[j] = 0.0;
                    lvd[j] = d;
                    for (int i = 0; i < 6; i++) Sst[j][i] = Sv[i];
                }
        }
        double F[6] = {0, 0, 0, 0, 0, 0};
        link(l, depth, out, Sst, lvd, F);
        if (ACC) {
            for (int i = 0; i < 6; i++) T[i] += F[i];
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int j = 0; j < MAXD; j++)
                if (j < depth) tac[j] += fbr_dot6(Sst[j], F);
        }
    }
    if (ACC) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < MAXD; j++)
            if (j < maxlvl) {
                const int fd = FBR_UNI(endflush[j]);
                if (fd >= 0) emit(fb + fd, tac[j]);
            }
        for (int r = 0; r < fb; r++) emit(r, T[r]);
    }
}

// Score of one regressor evaluation against a weight block (fbr_fd_scores, analyticalGradient.py:92-185):  the contribution of link l's
// inertial columns c = cpl l + p,  sum_r W[r][c] Y[r][c]  with Y's base rows = the unit wrench, joint row of path joint j = S_j . unit wrench.
// Wr(r, c): the weight of regressor row r, column c of this lane's sample.
template <int MAXD, class WFn>
FBR_HD double fbr_kinfd_link_score(int l, int depth, const double *rec, const double (*Sst)[6], const int *lvd, int cpl, int fb, WFn Wr)
{
    double acc = 0.0;
#if defined(__HIPCC__)
#pragma unroll  // (the parameter index must be a constant: fbr_unit_wrench indexes small arrays with it)
#endif
    for (int p = 0; p < 10; p++)
        if (p < cpl) {
            const int c = cpl * l + p;
            double w6[6];
            fbr_unit_wrench(rec, p, w6);
            for (int r = 0; r < fb; r++) acc += Wr(r, c) * w6[r];
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int j = 0; j < MAXD; j++)
                if (j < depth) acc += Wr(fb + lvd[j], c) * fbr_dot6(Sst[j], w6);
        }
    return acc;
}

#if defined(__HIPCC__)
struct DevKinId {
    int nsteps, maxlvl, nslots, ldn;  // ldn: row stride (doubles, odd) of the staged joint states of one sample
    const int *steps, *endflush;
};
// candidate extrema (fbr_candidate_extrema): C candidates of T consecutive samples each, cut into tiles of 64 samples that never span two
// candidates (tiles = ceil(T / 64) per candidate, tile b = candidate b / tiles).  Every tile writes [4][n] (value, index) partials --
// 0 min q, 1 max q, 2 max |dq|, 3 max |nan_to_num(tau)| over the joint rows -- the index counted inside the candidate; the finishing kernel
// reduces a candidate's tiles in tile order (no atomics: deterministic).
struct DevKinExt {
    long T, tiles, nblk;  // samples per candidate, tiles per candidate, tiles in all
    double *val;          // [nblk][4][n]
    long *idx;            // [nblk][4][n]
};
// value of quantity k that the extrema compare: q as is, |dq|, |nan_to_num(tau)| (NaN -> 0, +-inf -> DBL_MAX: what np.nan_to_num hands on)
FBR_HD double fbr_ext_value(int k, double v)
{
    if (k == 2) return fabs(v);
    if (k == 3) return v != v ? 0.0 : fmin(fabs(v), 1.7976931348623157e308);
    return v;
}
// does a LATER sample's value a replace the running extremum b (k == 0: minimum, else maximum)?  NumPy's rules: the first NaN wins and
// stays, ties keep the earlier index
FBR_HD bool fbr_ext_take(int k, double a, double b)
{
    if (b != b) return false;
    return a != a || (k == 0 ? a < b : a > b);
}
// tables of the lane WRITERS (fbr_kinwrite_kernel below, fbr_kinimg_kernel in fbr_gram64.h)
// destinations arrive as integers: a pointer made from one is GENERIC (flat_store: counted by lgkmcnt as well, so that every wait for a scalar load
// or an LDS read would also wait for the stores in flight) unless it is given the global address space explicitly
typedef __attribute__((address_space(1))) char *fbr_gchar_ptr;
typedef __attribute__((address_space(1))) double *fbr_gdouble_ptr;
struct DevKinWrite {
    const int *lcol10, *colrec;  // lcol10 [parts][10 L]: the columns a part's wave writes; colrec [cols + 1][2]
    const int *lanecol = nullptr;  // (fbr_kinimg_kernel) [parts][L][64]: the running sum a lane adds a link's moment to (fbr_gram64_lane_columns)
    const long *dst;
    int ninert, cols, k, has_w;
    int flev;  // (fbr_kinimg_kernel) base rows below this level go through the force-tile words
    int base_only;  // (fbr_kinimg_kernel) the joint rows carry weight 0 in every sample: not produced
    long group_samples;  // (fbr_kinimg_kernel) samples per group of a grouped pass (every group starts a block), 0: one group
    const int *none = nullptr;  // (fbr_kinimg_kernel) [parts][L]: 1 = the part writes no column of the link (FbrGram64Producer::none); null: not consulted
    int nparts, part_nsteps[FBR_KINWRITE_PARTS], part_step0[FBR_KINWRITE_PARTS];  // wave w of a workgroup walks steps [step0, step0 + nsteps) of p.steps
};
#endif

#if defined(__HIPCC__) && defined(FBR_KERNELS_CORE)

// mode 0: x = full standard vector (10 per link + friction slots); mode 1: x = identified-parameter vector (cols);
// mode 2: contact wrench -> generalized force J^T w (fbr_contact_torques, model.py:535-555): x = [S][6] wrenches at the frame
// (link `flink`, point fpx/y/z in its axes), every other link contributes nothing, no friction.
// grid-stride over blocks of 64 samples; dynamic LDS: 3 x [64][ldn] doubles (q, dq, ddq of the wave's samples).
// scratch: [gridDim.x][nslots][FBR_LINK_REC][64] doubles.
// EXT (fbr_candidate_extrema, mode 0): blocks of 64 samples of ONE candidate (DevKinExt); `emit` puts a sample's joint torques into the
// LDS (over its staged ddq, read by then) instead of HBM, and the block's extrema of q, |dq| and |tau| are scanned from the LDS after the
// lane body -- nothing per sample leaves the CU.  The lane body and `emit`'s arithmetic are the plain instance's: the torques compared are
// the ones fbr_inverse_dynamics_batch returns, bit for bit.
// friction torque of joint d from the standard-parameter vector (mode 0, model.py:299-326): Coulomb, and unless gravity-only the viscous
// term, the constant offset and the Stribeck term; vs: the joint's vel_sign entry, read under Stribeck friction only
__device__ __forceinline__ double fbr_friction_std(const DevModel &m, const double *__restrict__ x, int d, double dqv, double sg, const double *vs)
{
    const int n = m.n;
    double t = sg * x[m.fstart + d];
    if (!m.grav_only) {
        t += x[m.fstart + n + d] * dqv;
        const int poff = m.fstart + 2 * n;
        t += x[poff + d];
        if (m.stribeck > 0) {
            const double sgn = (sg > 0) - (sg < 0);
            t += x[poff + n + d] * exp(-fabs(*vs) / m.stribeck) * sgn;
        }
    }
    return t;
}

template <int MAXD, bool EXT = false>
__global__ __launch_bounds__(64) void fbr_kinid_kernel(DevModel m, DevKinId p, long S, const double *__restrict__ q, const double *__restrict__ dq,
                                                       const double *__restrict__ ddq, const double *__restrict__ bv,
                                                       const double *__restrict__ ba, const double *__restrict__ rpy,
                                                       const double *__restrict__ sign, const double *__restrict__ vel_sign,
                                                       const double *__restrict__ x, int mode, double *__restrict__ tau, double *__restrict__ scratch, int flink, double fpx,
                                                       double fpy, double fpz, DevKinExt ex)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x, n = m.n, ldn = p.ldn;
    double *sq = smem, *sdq = sq + 64 * ldn, *sddq = sdq + 64 * ldn;
    double *scr = scratch + (long)blockIdx.x * p.nslots * FBR_LINK_REC * 64 + lane;
    const long nblk = EXT ? ex.nblk : (S + 63) >> 6;
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        long base, i0 = 0;  // i0 (EXT): index of the block's first sample inside its candidate
        int valid;
        if constexpr (EXT) {
            const long c = blk / ex.tiles;
            i0 = (blk - c * ex.tiles) << 6;
            base = c * ex.T + i0;
            valid = (int)min(64L, ex.T - i0);
        } else {
            base = blk << 6;
            valid = (int)min(64L, S - base);
        }
        __syncthreads();  // (the block before has read its states)
        {
            // coalesced copy of the block's q / dq / ddq rows into [sample][ldn]
            const long off = base * n;
            const int cnt = valid * n;
            int sr = lane / n, dc = lane - sr * n;
            const int ds = 64 / n, dd = 64 - ds * n;
            for (int i = lane; i < cnt; i += 64) {
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
        }
        __syncthreads();
        const int ls = min(lane, valid - 1);  // lanes behind the last sample repeat it and store nothing
        const long s = base + ls;
        const bool live = lane < valid;
        const double *mysq = sq + ls * ldn, *mysdq = sdq + ls * ldn, *mysddq = sddq + ls * ldn;
        double *ts = tau + s * m.rows;
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
        auto link = [&](int l, int depth, const double *rec, const double (*Sst)[6], const int *lvd, double *F) {
            (void)depth; (void)Sst; (void)lvd;
            if (mode == 2) {
                if (l != flink) return;
                const double *w = x + s * 6;
                const double fp[3] = {fpx, fpy, fpz};
                double t[3], pf[3], f[3] = {w[0], w[1], w[2]}, pxf[3];
                fbr_mv(rec + FBR_OFF_R, fp, t);
                for (int i = 0; i < 3; i++) pf[i] = rec[FBR_OFF_P + i] + t[i];
                fbr_cross(pf, f, pxf);
                for (int i = 0; i < 3; i++) {
                    F[i] = f[i];
                    F[3 + i] = w[3 + i] + pxf[i];  // the wrench about the base origin (frame A)
                }
                return;
            }
            double pi[10];
            if (mode == 0) {
                for (int c = 0; c < 10; c++) pi[c] = x[10 * l + c];
            } else {
                for (int c = 0; c < 10; c++) pi[c] = (c < m.cpl) ? x[m.cpl * l + c] : 0.0;
            }
            fbr_link_wrench(rec, pi, F);
        };
        auto consts = [&](int l, double *rR, double *rp, double *ax) {  // (l is wave-uniform: scalar loads through the constant address space)
            const fbr_cdouble_ptr cR = (fbr_cdouble_ptr)(unsigned long)m.restR, cp = (fbr_cdouble_ptr)(unsigned long)m.restp,
                                  ca = (fbr_cdouble_ptr)(unsigned long)m.axis;
            for (int i = 0; i < 9; i++) rR[i] = cR[9 * l + i];
            for (int i = 0; i < 3; i++) {
                rp[i] = cp[3 * l + i];
                ax[i] = ca[3 * l + i];
            }
        };
        auto emit = [&](int r, double v) {
            if (r >= m.fb && m.fric && mode != 2) {
                const int d = r - m.fb;
                const double dqv = mysdq[d];
                const double sg = sign[s * n + d];
                if (mode == 0) {
                    v += fbr_friction_std(m, x, d, dqv, sg, vel_sign + s * n + d);
                } else {
                    for (int c = m.cpl * m.L; c < m.cols; c++) {
                        const int4 cd = m.coldesc[c];
                        if (cd.w == d) v += x[c] * fbr_friction_value(cd.z, dqv, sg, m.stribeck);
                    }
                }
            }
            if constexpr (EXT) {
                // the joint row goes into the lane's own staged ddq entry of that joint: the joint's link has read it (a joint's torque is
                // complete only after every link below it has been walked), nothing reads it again
                if (r >= m.fb && live) sddq[lane * ldn + r - m.fb] = v;
            } else if (live) {
                ts[r] = v;
            }
        };
        fbr_kinid_lane<MAXD, true>(p.nsteps, p.maxlvl, p.steps, p.endflush, m.floating, m.g, m.fb, state, basest, save, load, link, emit, consts);
        if constexpr (EXT) {
            // one lane per joint scans the block's rows in sample order (ties keep the first): q and dq as staged, the torques where emit
            // left them
            __syncthreads();
            double *pv = ex.val + blk * 4 * n;
            long *pi = ex.idx + blk * 4 * n;
            for (int d = lane; d < n; d += 64) {
                // plain comparisons (a NaN compares false: it is never taken), the NaN rules of fbr_ext_take only for a column that has
                // one past its first row; a NaN torque counts as 0, which the running maximum (>= 0 from the first row on) never takes
                double b[4] = {sq[d], sq[d], fbr_ext_value(2, sdq[d]), fbr_ext_value(3, sddq[d])};
                int ib[4] = {0, 0, 0, 0};
                bool nan = false;
                for (int r = 1; r < valid; r++) {
                    const double aq = sq[r * ldn + d], ad = fabs(sdq[r * ldn + d]), at = sddq[r * ldn + d];
                    const double ct = fmin(fabs(at), 1.7976931348623157e308);
                    nan |= __builtin_isunordered(aq, ad);
                    if (aq < b[0]) b[0] = aq, ib[0] = r;
                    if (aq > b[1]) b[1] = aq, ib[1] = r;
                    if (ad > b[2]) b[2] = ad, ib[2] = r;
                    if (ct > b[3] && at == at) b[3] = ct, ib[3] = r;
                }
                if (nan) {
                    b[0] = b[1] = sq[d];
                    b[2] = fbr_ext_value(2, sdq[d]);
                    ib[0] = ib[1] = ib[2] = 0;
                    for (int r = 1; r < valid; r++) {
                        const double aq = sq[r * ldn + d], ad = fbr_ext_value(2, sdq[r * ldn + d]);
                        if (fbr_ext_take(0, aq, b[0])) b[0] = aq, ib[0] = r;
                        if (fbr_ext_take(1, aq, b[1])) b[1] = aq, ib[1] = r;
                        if (fbr_ext_take(2, ad, b[2])) b[2] = ad, ib[2] = r;
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    pv[k * n + d] = b[k];
                    pi[k * n + d] = i0 + ib[k];
                }
            }
        }
    }
}
// Candidate extrema from MATERIALISED states and torques (the two-kernel route of fbr_candidate_extrema: fused_id = 0, joint paths beyond
// FBR_KINID_MAXD, more than 105 DOF): the tiles and partials of the EXT instance above.  A workgroup per tile, a thread per (quantity,
// joint) scans the tile's samples in order; tau [S][rows], the joint rows from fb on.
__global__ __launch_bounds__(256) void fbr_extrema_tiles_kernel(DevKinExt ex, int n, int fb, int rows, const double *__restrict__ q,
                                                                const double *__restrict__ dq, const double *__restrict__ tau)
{
    for (long blk = blockIdx.x; blk < ex.nblk; blk += gridDim.x) {
        const long c = blk / ex.tiles, i0 = (blk - c * ex.tiles) << 6, base = c * ex.T + i0;
        const int valid = (int)min(64L, ex.T - i0);
        for (int kd = threadIdx.x; kd < 4 * n; kd += blockDim.x) {
            const int k = kd / n, d = kd - k * n;
            const double *src = k < 2 ? q + base * n + d : k == 2 ? dq + base * n + d : tau + base * rows + fb + d;
            const long ld = k < 3 ? n : rows;
            double b = fbr_ext_value(k, src[0]);
            int ib = 0;
            for (int r = 1; r < valid; r++) {
                const double a = fbr_ext_value(k, src[r * ld]);
                if (fbr_ext_take(k, a, b)) b = a, ib = r;
            }
            ex.val[blk * 4 * n + kd] = b;
            ex.idx[blk * 4 * n + kd] = i0 + ib;
        }
    }
}
// the partials of a candidate's tiles reduced in tile order: out [C][4][n], one thread per entry
__global__ __launch_bounds__(256) void fbr_extrema_finish_kernel(DevKinExt ex, int n, long C, double *__restrict__ val, long *__restrict__ idx)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= C * 4 * n) return;
    const long c = t / (4 * n);
    const int kd = (int)(t - c * 4 * n), k = kd / n;
    const double *v = ex.val + c * ex.tiles * 4 * n + kd;
    const long *ix = ex.idx + c * ex.tiles * 4 * n + kd;
    double b = v[0];
    long ib = ix[0];
#pragma unroll 8
    for (long j = 1; j < ex.tiles; j++) {
        const double a = v[j * 4 * n];
        if (fbr_ext_take(k, a, b)) b = a, ib = ix[j * 4 * n];
    }
    val[t] = b;
    idx[t] = ib;
}
// Finite-difference sweep (analyticalGradient.py:92-185): one lane per EVALUATION e = s (1 + 3 n) + j -- j = 0 the state of
// sample s itself, 1 + kind n + d the state with +eps on q_d / dq_d / ddq_d -- score[e] = sum_{r,c} W_s[r][c] Y_e[r][c], the regressor
// never stored, no records, no expanded states in memory.  The lanes of a wave share one or two samples: their weights arrive as
// broadcast loads.  (The two-kernel path it replaces evaluates a perturbation's sub-tree columns only but stages every evaluation's
// kinematic records through HBM and the LDS of a whole workgroup: latency bound at 0.01 of its HBM floor.)
template <int MAXD>
__global__ __launch_bounds__(64) void fbr_kinfd_kernel(DevModel m, DevKinId p, long S, int nper, double eps, const double *__restrict__ q,
                                                       const double *__restrict__ dq, const double *__restrict__ ddq, const double *__restrict__ bv,
                                                       const double *__restrict__ ba, const double *__restrict__ rpy, const double *__restrict__ sign,
                                                       const double *__restrict__ W, double *__restrict__ out, double *__restrict__ scratch)
{
    const int lane = threadIdx.x, n = m.n;
    double *scr = scratch + (long)blockIdx.x * p.nslots * FBR_LINK_REC * 64 + lane;
    const long total = S * nper, nblk = (total + 63) >> 6;
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long e = min((blk << 6) + lane, total - 1);
        const bool live = (blk << 6) + lane < total;
        const long s = e / nper;
        const int j = (int)(e - s * nper);
        const int kind = (j == 0) ? -1 : (j - 1) / n, dj = (j == 0) ? -1 : (j - 1) % n;
        const double *Ws = W + s * (long)m.rows * m.cols;
        double score = 0.0;
        auto state = [&](int d, double &a, double &b, double &c) {
            a = q[s * n + d] + ((kind == 0 && d == dj) ? eps : 0.0);
            b = dq[s * n + d] + ((kind == 1 && d == dj) ? eps : 0.0);
            c = ddq[s * n + d] + ((kind == 2 && d == dj) ? eps : 0.0);
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
        auto Wr = [&](int r, int c) { return Ws[(long)r * m.cols + c]; };
        auto link = [&](int l, int depth, const double *rec, const double (*Sst)[6], const int *lvd, double *F) {
            (void)F;
            score += fbr_kinfd_link_score<MAXD>(l, depth, rec, Sst, lvd, m.cpl, m.fb, Wr);
        };
        auto emit = [&](int, double) {};
        fbr_kinid_lane<MAXD, false>(p.nsteps, p.maxlvl, p.steps, p.endflush, m.floating, m.g, m.fb, state, basest, save, load, link, emit, consts);
        for (int c = m.cpl * m.L; c < m.cols; c++) {  // friction columns: one entry each
            const int4 cd = m.coldesc[c];
            const int jj = cd.w;
            const double dqv = dq[s * n + jj] + ((kind == 1 && jj == dj) ? eps : 0.0);
            score += Ws[(long)(m.fb + jj) * m.cols + c] * fbr_friction_value(cd.z, dqv, sign ? sign[s * n + jj] : 0.0, m.stribeck);
        }
        if (live) out[e] = score;
    }
}
// Torque rows under the same sweep (fbr_torque_row_sweep; analyticalGradient.py:114-183 at the sample where |tau_n| peaks): one lane per
// EVALUATION e = item (1 + 3 n) + j of item = (candidate c, row r) -- sample tr.sample[item] of candidate c, state perturbed as in
// fbr_kinfd_kernel -- out[e] = joint torque row tr.joint[item] (NULL: r) of the inverse dynamics of x (mode 0 of fbr_kinid_kernel: the same
// lane body, link wrench and friction term; the sign series, vel_sign and the base state stay the sample's own).  Nothing is expanded in
// memory; every other row the lane body emits is dropped.  An index outside its range is read clamped and raises *tr.flag.
struct DevKinTau {
    long T, R;           // samples per candidate, rows per candidate
    const long *sample;  // [C][R]
    const int *joint;    // [C][R] or NULL
    int *flag;
};
template <int MAXD>
__global__ __launch_bounds__(64) void fbr_kintau_kernel(DevModel m, DevKinId p, DevKinTau tr, long items, int nper, double eps, const double *__restrict__ q,
                                                        const double *__restrict__ dq, const double *__restrict__ ddq, const double *__restrict__ bv,
                                                        const double *__restrict__ ba, const double *__restrict__ rpy, const double *__restrict__ sign,
                                                        const double *__restrict__ vel_sign, const double *__restrict__ x, double *__restrict__ out,
                                                        double *__restrict__ scratch)
{
    const int lane = threadIdx.x, n = m.n;
    double *scr = scratch + (long)blockIdx.x * p.nslots * FBR_LINK_REC * 64 + lane;
    const long total = items * nper, nblk = (total + 63) >> 6;
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long e = min((blk << 6) + lane, total - 1);
        const bool live = (blk << 6) + lane < total;
        const long item = e / nper, c = item / tr.R;
        const int j = (int)(e - item * nper);
        const int kind = (j == 0) ? -1 : (j - 1) / n, dj = (j == 0) ? -1 : (j - 1) % n;
        const long smp = tr.sample[item], smpc = min(max(smp, 0L), tr.T - 1);
        const int jn = tr.joint ? tr.joint[item] : (int)(item - c * tr.R), jnc = min(max(jn, 0), n - 1);
        if ((smp != smpc || jn != jnc) && live) *tr.flag = 1;
        const long s = c * tr.T + smpc;
        double row = 0.0;
        auto state = [&](int d, double &a, double &b, double &cc) {
            a = q[s * n + d] + ((kind == 0 && d == dj) ? eps : 0.0);
            b = dq[s * n + d] + ((kind == 1 && d == dj) ? eps : 0.0);
            cc = ddq[s * n + d] + ((kind == 2 && d == dj) ? eps : 0.0);
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
        auto link = [&](int l, int depth, const double *rec, const double (*Sst)[6], const int *lvd, double *F) {
            (void)depth; (void)Sst; (void)lvd;
            double pi[10];
            for (int i = 0; i < 10; i++) pi[i] = x[10 * l + i];
            fbr_link_wrench(rec, pi, F);
        };
        auto emit = [&](int r, double v) {
            if (r != m.fb + jnc) return;
            if (m.fric) {
                const double dqv = dq[s * n + jnc] + ((kind == 1 && jnc == dj) ? eps : 0.0);
                v += fbr_friction_std(m, x, jnc, dqv, sign[s * n + jnc], vel_sign + s * n + jnc);
            }
            row = v;
        };
        fbr_kinid_lane<MAXD, true>(p.nsteps, p.maxlvl, p.steps, p.endflush, m.floating, m.g, m.fb, state, basest, save, load, link, emit, consts);
        if (live) out[e] = row;
    }
}
// The two-kernel route of the same sweep (fused_id = 0, joint paths beyond FBR_KINID_MAXD, more than 105 DOF): the perturbed states of the
// items [i0, i0 + ci) written out for fbr_kin_kernel + fbr_id_kernel (one thread per evaluation; es / evs only with friction / Stribeck) ...
__global__ __launch_bounds__(256) void fbr_tau_expand_kernel(DevKinTau tr, long i0, long ci, int n, double eps, const double *__restrict__ q,
                                                             const double *__restrict__ dq, const double *__restrict__ ddq, const double *__restrict__ bv,
                                                             const double *__restrict__ ba, const double *__restrict__ rpy, const double *__restrict__ sign,
                                                             const double *__restrict__ vel_sign, double *__restrict__ eq, double *__restrict__ edq,
                                                             double *__restrict__ eddq, double *__restrict__ ebv, double *__restrict__ eba,
                                                             double *__restrict__ erpy, double *__restrict__ es, double *__restrict__ evs)
{
    const int nper = 1 + 3 * n;
    const long total = ci * nper;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long item = i0 + e / nper, c = item / tr.R;
        const int j = (int)(e % nper);
        const int kind = (j == 0) ? -1 : (j - 1) / n, dj = (j == 0) ? -1 : (j - 1) % n;
        const long smp = tr.sample[item], smpc = min(max(smp, 0L), tr.T - 1);
        if (smp != smpc) *tr.flag = 1;
        const long s = c * tr.T + smpc;
        for (int i = 0; i < n; i++) {
            eq[e * n + i] = q[s * n + i] + ((kind == 0 && i == dj) ? eps : 0.0);
            edq[e * n + i] = dq[s * n + i] + ((kind == 1 && i == dj) ? eps : 0.0);
            eddq[e * n + i] = ddq[s * n + i] + ((kind == 2 && i == dj) ? eps : 0.0);
            if (sign) es[e * n + i] = sign[s * n + i];
            if (vel_sign) evs[e * n + i] = vel_sign[s * n + i];
        }
        if (bv) {
            for (int i = 0; i < 6; i++) {
                ebv[e * 6 + i] = bv[s * 6 + i];
                eba[e * 6 + i] = ba[s * 6 + i];
            }
            for (int i = 0; i < 3; i++) erpy[e * 3 + i] = rpy[s * 3 + i];
        }
    }
}
// ... and the requested rows gathered from their torques tau [ci (1 + 3 n)][rows]
__global__ __launch_bounds__(256) void fbr_tau_gather_kernel(DevKinTau tr, long i0, long ci, int n, int fb, int rows, const double *__restrict__ tau,
                                                             double *__restrict__ out)
{
    const int nper = 1 + 3 * n;
    const long total = ci * nper;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long item = i0 + e / nper;
        const int jn = tr.joint ? tr.joint[item] : (int)(item % tr.R), jnc = min(max(jn, 0), n - 1);
        if (jn != jnc) *tr.flag = 1;
        out[i0 * nper + e] = tau[e * rows + fb + jnc];
    }
}

// ------------------------------------------------------------------------------------------------
// Suspended base (fbr_suspended_base_motion; excitation/suspendedDynamics.py simulate_suspended_base_motion): the robot hangs from a ball
// joint at the origin O of the attachment link.  Per sample, the moment about O that inverse dynamics asks for, in the attachment's axes, is
//     N = c0 + B w + w x (I w) + I dw - mc x u        (w, dw: the attachment's angular velocity / acceleration in its own axes, u = R^T g)
// with I, B, c0, mc functions of the sample's (q, dq, ddq) and the parameters only.  fbr_kinsusp_kernel writes them, with the base
// link's pose and twist relative to the attachment frame, as a record of FBR_SUSP_REC doubles per sample; fbr_susp_scan_kernel then steps
// every candidate through its records at O(1) per step.
//
// One lane per sample on the lane body: a walk down the attachment's path with the base at rest gives the attachment's pose, velocity and
// acceleration relative to the base; four full walks at zero gravity follow, the base link in the state that holds the attachment frame at
// O with zero linear velocity / acceleration, zero angular acceleration and angular velocity 0, e_x, e_y, e_z (its own axes).  Their base
// rows, moved to O and turned into the attachment's axes, are c0 and c0 + B e_i + e_i x I e_i; I and mc are sums over the link records of
// the first full walk.  The walks run in the BASE link's axes (base orientation 1): the lane body needs no rpy of a rotation matrix then.
// ------------------------------------------------------------------------------------------------
struct DevKinSusp {
    int att;             // the attachment link
    int nsteps, maxlvl;  // the program that walks the attachment's path only (fbr_kinid_build with keep = the link and its ancestors)
    const int *steps;
};
template <int MAXD>
__global__ __launch_bounds__(64) void fbr_kinsusp_kernel(DevModel m, DevKinId p, DevKinSusp su, long S, const double *__restrict__ q,
                                                         const double *__restrict__ dq, const double *__restrict__ ddq, const double *__restrict__ x,
                                                         double *__restrict__ rec, double *__restrict__ scratch)
{
    const int lane = threadIdx.x, n = m.n;
    double *scr = scratch + (long)blockIdx.x * p.nslots * FBR_LINK_REC * 64 + lane;
    const long nblk = (S + 63) >> 6;
    const double g0[3] = {0.0, 0.0, 0.0};
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long s = min((blk << 6) + lane, S - 1);
        const bool live = (blk << 6) + lane < S;
        auto state = [&](int d, double &a, double &b, double &c) {
            a = q[s * n + d];
            b = dq[s * n + d];
            c = ddq[s * n + d];
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
        // ---- the attachment relative to the base: Ra, pa (pose), wa, dwa (its own axes), va, aa (origin, base axes)
        double Ra[9], pa[3], wa[3], dwa[3], va[3], aa[3];
        for (int i = 0; i < 9; i++) Ra[i] = (i % 4 == 0) ? 1.0 : 0.0;
        for (int i = 0; i < 3; i++) pa[i] = wa[i] = dwa[i] = va[i] = aa[i] = 0.0;
        {
            auto basest = [&](double *, double *, double *) {};
            auto link = [&](int l, int depth, const double *r, const double (*Sst)[6], const int *lvd, double *F) {
                (void)F;
                if (l != su.att) return;
                for (int i = 0; i < 9; i++) Ra[i] = r[FBR_OFF_R + i];
                double tw[6] = {0, 0, 0, 0, 0, 0}, t[3];
                for (int i = 0; i < 3; i++) {
                    pa[i] = r[FBR_OFF_P + i];
                    wa[i] = r[FBR_OFF_W + i];
                    dwa[i] = r[FBR_OFF_DW + i];
                }
                fbr_mv(Ra, r + FBR_OFF_A, aa);  // (zero gravity, base at rest: the proper acceleration is the acceleration)
#pragma unroll
                for (int j = 0; j < MAXD; j++)
                    if (j < depth) {
                        const double dqj = dq[s * n + lvd[j]];
                        for (int i = 0; i < 6; i++) tw[i] += Sst[j][i] * dqj;
                    }
                fbr_cross(tw + 3, pa, t);
                for (int i = 0; i < 3; i++) va[i] = tw[i] + t[i];
            };
            auto emit = [&](int, double) {};
            fbr_kinid_lane<MAXD, false>(su.nsteps, su.maxlvl, su.steps, p.endflush, 0, g0, 0, state, basest, save, load, link, emit, consts);
        }
        double wrel[3], arel[3];
        fbr_mv(Ra, wa, wrel);
        fbr_mv(Ra, dwa, arel);
        // ---- four probes; the first one also sums the composite inertia and first moment about O (base axes)
        double Nk[12], Io[6] = {0, 0, 0, 0, 0, 0}, mc[3] = {0, 0, 0};
#pragma nounroll
        for (int k = 0; k < 4; k++) {
            double om[3], wB[3], dwB[3], aB[3], t1[3], t2[3], t3[3], T6[6] = {0, 0, 0, 0, 0, 0};
            for (int i = 0; i < 3; i++) om[i] = ((k == i + 1) ? 1.0 : 0.0) - wa[i];
            fbr_mv(Ra, om, wB);
            fbr_cross(wB, wrel, t1);
            for (int i = 0; i < 3; i++) dwB[i] = -t1[i] - arel[i];
            fbr_cross(dwB, pa, t1);
            fbr_cross(wB, pa, t2);
            fbr_cross(wB, t2, t3);
            fbr_cross(wB, va, t2);
            for (int i = 0; i < 3; i++) aB[i] = -(t1[i] + t3[i] + 2.0 * t2[i] + aa[i]);
            auto basest = [&](double *v6, double *a6, double *e3) {
                for (int i = 0; i < 3; i++) {
                    v6[i] = 0.0;
                    v6[3 + i] = wB[i];
                    a6[i] = aB[i];
                    a6[3 + i] = dwB[i];
                    e3[i] = 0.0;
                }
            };
            auto link = [&](int l, int depth, const double *r, const double (*Sst)[6], const int *lvd, double *F) {
                (void)depth; (void)Sst; (void)lvd;
                double pi[10];
                for (int i = 0; i < 10; i++) pi[i] = x[10 * l + i];
                fbr_link_wrench(r, pi, F);
                if (k == 0) {
                    const double *R = r + FBR_OFF_R;
                    double d[3], h[3];
                    for (int i = 0; i < 3; i++) d[i] = r[FBR_OFF_P + i] - pa[i];
                    fbr_mv(R, pi + 1, h);
                    for (int i = 0; i < 3; i++) mc[i] += pi[0] * d[i] + h[i];
                    // R Ibar R^T, then the shift of the reference point from the link origin to O by d
                    const double Ib[9] = {pi[4], pi[5], pi[6], pi[5], pi[7], pi[8], pi[6], pi[8], pi[9]};
                    double RI[9];
                    fbr_mm(R, Ib, RI);
                    const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], dh = d[0] * h[0] + d[1] * h[1] + d[2] * h[2];
                    int e = 0;
                    for (int a = 0; a < 3; a++)
                        for (int b = a; b < 3; b++, e++) {
                            double v = RI[3 * a] * R[3 * b] + RI[3 * a + 1] * R[3 * b + 1] + RI[3 * a + 2] * R[3 * b + 2];
                            v -= pi[0] * d[a] * d[b] + d[a] * h[b] + h[a] * d[b];
                            if (a == b) v += pi[0] * dd + 2.0 * dh;
                            Io[e] += v;
                        }
                }
            };
            auto emit = [&](int r, double v) {
#pragma unroll
                for (int i = 0; i < 6; i++)
                    if (r == i) T6[i] = v;
            };
            fbr_kinid_lane<MAXD, true>(p.nsteps, p.maxlvl, p.steps, p.endflush, 1, g0, 6, state, basest, save, load, link, emit, consts);
            fbr_cross(pa, T6, t1);
            for (int i = 0; i < 3; i++) t2[i] = T6[3 + i] - t1[i];  // the moment about O (base axes) ...
            fbr_mtv(Ra, t2, t3);                                     // ... in the attachment's axes
#pragma unroll
            for (int kk = 0; kk < 4; kk++)
                if (kk == k)
                    for (int i = 0; i < 3; i++) Nk[3 * kk + i] = t3[i];
        }
        // ---- the record
        double out[FBR_SUSP_REC];
        {
            const double If[9] = {Io[0], Io[1], Io[2], Io[1], Io[3], Io[4], Io[2], Io[4], Io[5]};
            double IR[9], Ia[9];
            fbr_mm(If, Ra, IR);
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) Ia[3 * a + b] = Ra[a] * IR[b] + Ra[3 + a] * IR[3 + b] + Ra[6 + a] * IR[6 + b];  // Ra^T I Ra
            out[FBR_SUSP_I + 0] = Ia[0];
            out[FBR_SUSP_I + 1] = 0.5 * (Ia[1] + Ia[3]);
            out[FBR_SUSP_I + 2] = 0.5 * (Ia[2] + Ia[6]);
            out[FBR_SUSP_I + 3] = Ia[4];
            out[FBR_SUSP_I + 4] = 0.5 * (Ia[5] + Ia[7]);
            out[FBR_SUSP_I + 5] = Ia[8];
            const double Is[9] = {out[0], out[1], out[2], out[1], out[3], out[4], out[2], out[4], out[5]};
            for (int i = 0; i < 3; i++) out[FBR_SUSP_C0 + i] = Nk[i];
            for (int c = 0; c < 3; c++) {
                // B e_c = N(e_c) - c0 - e_c x (I e_c)
                const double e[3] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0}, Ie[3] = {Is[c], Is[3 + c], Is[6 + c]};
                double ex[3];
                fbr_cross(e, Ie, ex);
                for (int r = 0; r < 3; r++) out[FBR_SUSP_B + 3 * r + c] = Nk[3 * (c + 1) + r] - Nk[r] - ex[r];
            }
            fbr_mtv(Ra, mc, out + FBR_SUSP_MC);
            double t[3], u[3];
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) out[FBR_SUSP_R + 3 * a + b] = Ra[3 * b + a];
            fbr_mtv(Ra, pa, t);
            for (int i = 0; i < 3; i++) out[FBR_SUSP_P + i] = -t[i];
            // the base link relative to the attachment frame: angular velocity -wa, origin velocity (-wa) x p_rel - Ra^T va
            fbr_mtv(Ra, va, t);
            const double wr[3] = {-wa[0], -wa[1], -wa[2]};
            fbr_cross(wr, out + FBR_SUSP_P, u);
            for (int i = 0; i < 3; i++) {
                out[FBR_SUSP_V + i] = u[i] - t[i];
                out[FBR_SUSP_V + 3 + i] = wr[i];
            }
        }
        if (live)
            for (int i = 0; i < FBR_SUSP_REC; i++) rec[s * FBR_SUSP_REC + i] = out[i];
    }
}

// rotation Rz(y) Ry(p) Rx(r) (iDynTree Rotation::RPY), row-major
FBR_HD void fbr_susp_rpy_R(const double *e, double *R)
{
    const double cr = cos(e[0]), sr = sin(e[0]), cp = cos(e[1]), sp = sin(e[1]), cy = cos(e[2]), sy = sin(e[2]);
    R[0] = cy * cp;
    R[1] = cy * sp * sr - sy * cr;
    R[2] = cy * sp * cr + sy * sr;
    R[3] = sy * cp;
    R[4] = sy * sp * sr + cy * cr;
    R[5] = sy * sp * cr - cy * sr;
    R[6] = -sp;
    R[7] = cp * sr;
    R[8] = cp * cr;
}
// x = M^-1 b for a symmetric 3 x 3 M (the cofactor form: no pivoting, no branch; M = R I R^T + d dt 1 is positive definite)
FBR_HD void fbr_susp_solve3(const double *M, const double *b, double *x)
{
    const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    const double c11 = M[0] * M[8] - M[2] * M[6], c12 = M[1] * M[6] - M[0] * M[7], c22 = M[0] * M[4] - M[1] * M[3];
    const double inv = 1.0 / (M[0] * c00 + M[1] * c01 + M[2] * c02);
    x[0] = (c00 * b[0] + c01 * b[1] + c02 * b[2]) * inv;
    x[1] = (c01 * b[0] + c11 * b[1] + c12 * b[2]) * inv;
    x[2] = (c02 * b[0] + c12 * b[1] + c22 * b[2]) * inv;
}
// the moment R (c0 + B w + w x (I w) - mc x (R^T g)) about O in world axes at angular velocity om (world), angular acceleration 0; rest:
// the static moment of the equilibrium search (zero joint velocities and accelerations: c0 and B drop out)
FBR_HD void fbr_susp_moment(const double *r39, const double *R, const double *om, const double *g, bool rest, double *Nw)
{
    double u[3], t[3], Nb[3];
    fbr_mtv(R, g, u);
    fbr_cross(r39 + FBR_SUSP_MC, u, t);
    for (int i = 0; i < 3; i++) Nb[i] = -t[i];
    if (!rest) {
        const double *I = r39 + FBR_SUSP_I, *B = r39 + FBR_SUSP_B;
        double w[3], Bw[3], wx[3];
        fbr_mtv(R, om, w);
        const double Iw[3] = {I[0] * w[0] + I[1] * w[1] + I[2] * w[2], I[1] * w[0] + I[3] * w[1] + I[4] * w[2], I[2] * w[0] + I[4] * w[1] + I[5] * w[2]};
        fbr_mv(B, w, Bw);
        fbr_cross(w, Iw, wx);
        for (int i = 0; i < 3; i++) Nb[i] += r39[FBR_SUSP_C0 + i] + Bw[i] + wx[i];
    }
    fbr_mv(R, Nb, Nw);
}
FBR_HD double fbr_susp_clip(double v, double lim) { return v > lim ? lim : (v < -lim ? -lim : v); }  // (a NaN stays a NaN)

// One lane per candidate: the equilibrium search on the record of its sample 0, then T steps of the reference's loop, each on one record
// (read a step ahead).  No cross-lane traffic; the loop bounds are T and FBR_SUSP_EQ_MAX_ITER.  att_state / info may be NULL.
__global__ __launch_bounds__(64) void fbr_susp_scan_kernel(long C, long T, double gx, double gy, double gz, double dt, double damping,
                                                           const double *__restrict__ rec, double *__restrict__ base_rpy, double *__restrict__ base_pos,
                                                           double *__restrict__ base_vel, double *__restrict__ att_state, long *__restrict__ info)
{
    const long c = (long)blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const double g[3] = {gx, gy, gz};
    const double *rc = rec + c * T * FBR_SUSP_REC;
    double cur[FBR_SUSP_REC];
    for (int i = 0; i < FBR_SUSP_REC; i++) cur[i] = rc[i];
    double e[3] = {0, 0, 0}, om[3] = {0, 0, 0}, R[9], Nw[3];
    const double eqlim = FBR_SUSP_EQ_CLIP_DEG * (M_PI / 180.0), swing = FBR_SUSP_MAX_SWING_DEG * (M_PI / 180.0);
    long iters = FBR_SUSP_EQ_MAX_ITER, clamps = 0;
    for (int it = 0; it < FBR_SUSP_EQ_MAX_ITER; it++) {
        fbr_susp_rpy_R(e, R);
        fbr_susp_moment(cur, R, om, g, true, Nw);
        if (sqrt(Nw[0] * Nw[0] + Nw[1] * Nw[1] + Nw[2] * Nw[2]) < FBR_SUSP_EQ_TOL) {
            iters = it + 1;
            break;
        }
        for (int i = 0; i < 3; i++) e[i] = fbr_susp_clip(e[i] - FBR_SUSP_EQ_STEP * Nw[i], eqlim);
    }
    for (long t = 0; t < T; t++) {
        double nxt[FBR_SUSP_REC];
        const double *rn = rc + min(t + 1, T - 1) * FBR_SUSP_REC;
        for (int i = 0; i < FBR_SUSP_REC; i++) nxt[i] = rn[i];
        const long s = c * T + t;
        fbr_susp_rpy_R(e, R);
        fbr_susp_moment(cur, R, om, g, false, Nw);
        // (M_bb + d dt 1) alpha = -(M_bj ddq + h_b) - d omega,  M_bb = R I R^T
        const double *I = cur + FBR_SUSP_I;
        const double If[9] = {I[0], I[1], I[2], I[1], I[3], I[4], I[2], I[4], I[5]};
        double RI[9], M[9], rhs[3], al[3];
        fbr_mm(R, If, RI);
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) M[3 * a + b] = RI[3 * a] * R[3 * b] + RI[3 * a + 1] * R[3 * b + 1] + RI[3 * a + 2] * R[3 * b + 2];
        M[1] = M[3] = 0.5 * (M[1] + M[3]);
        M[2] = M[6] = 0.5 * (M[2] + M[6]);
        M[5] = M[7] = 0.5 * (M[5] + M[7]);
        for (int i = 0; i < 3; i++) {
            M[4 * i] += damping * dt;
            rhs[i] = -Nw[i] - damping * om[i];
        }
        fbr_susp_solve3(M, rhs, al);
        // the base link before integrating: world_R_base = R R_rel, position R p_rel, twist [om x (R p_rel) + R v_rel; om + R w_rel]
        double Rb[9], pb[3], vl[3], va[3], t3[3];
        fbr_mm(R, cur + FBR_SUSP_R, Rb);
        fbr_mv(R, cur + FBR_SUSP_P, pb);
        fbr_mv(R, cur + FBR_SUSP_V, vl);
        fbr_mv(R, cur + FBR_SUSP_V + 3, va);
        fbr_cross(om, pb, t3);
        // rpy of world_R_base^T (iDynTree asRPY, general branch; at |R20| >= 1: pitch +-pi/2, roll 0, the whole turn about z in yaw)
        const double m20 = Rb[2], m21 = Rb[5], m22 = Rb[8], m10 = Rb[1], m00 = Rb[0];  // (entries of the transpose)
        double br, bp, by;
        if (fabs(m20) >= 1.0) {
            br = 0.0;
            bp = m20 < 0 ? 0.5 * M_PI : -0.5 * M_PI;
            by = atan2(-Rb[3], Rb[4]);
        } else {
            br = atan2(m21, m22);
            bp = asin(-m20);
            by = atan2(m10, m00);
        }
        base_rpy[s * 3] = br;
        base_rpy[s * 3 + 1] = bp;
        base_rpy[s * 3 + 2] = by;
        for (int i = 0; i < 3; i++) {
            base_pos[s * 3 + i] = pb[i];
            base_vel[s * 6 + i] = t3[i] + vl[i];
            base_vel[s * 6 + 3 + i] = om[i] + va[i];
        }
        if (att_state)
            for (int i = 0; i < 3; i++) {
                att_state[s * 6 + i] = e[i];
                att_state[s * 6 + 3 + i] = om[i];
            }
        if (t < T - 1) {
            // semi-implicit Euler; the rpy rates as angular_velocity_to_rpy_rates forms them: ((1 / cp) E) omega
            for (int i = 0; i < 3; i++) om[i] += al[i] * dt;
            const double cr = cos(e[0]), sr = sin(e[0]), cp = cos(e[1]), sp = sin(e[1]), ic = 1.0 / cp;
            const double d0 = (ic * cp) * om[0] + (ic * (sr * sp)) * om[1] + (ic * (cr * sp)) * om[2];
            const double d1 = (ic * 0.0) * om[0] + (ic * (cr * cp)) * om[1] + (ic * (-sr * cp)) * om[2];
            const double d2 = (ic * 0.0) * om[0] + (ic * sr) * om[1] + (ic * cr) * om[2];
            e[0] += d0 * dt;
            e[1] += d1 * dt;
            e[2] += d2 * dt;
            for (int i = 0; i < 3; i++) {
                if (e[i] > swing) {
                    e[i] = swing;
                    if (om[i] > 0) om[i] *= FBR_SUSP_BOUNCE;
                    clamps++;
                } else if (e[i] < -swing) {
                    e[i] = -swing;
                    if (om[i] < 0) om[i] *= FBR_SUSP_BOUNCE;
                    clamps++;
                }
            }
        }
        for (int i = 0; i < FBR_SUSP_REC; i++) cur[i] = nxt[i];
    }
    if (info) {
        info[2 * c] = iters;
        info[2 * c + 1] = clamps;
    }
}
// base_acc: central differences of base_vel with dt inside every candidate, one-sided at its two ends; zeros when T <= 2 (the reference's rule)
__global__ __launch_bounds__(256) void fbr_susp_acc_kernel(long C, long T, double dt, const double *__restrict__ vel, double *__restrict__ acc)
{
    const long total = C * T * 6;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long s = e / 6, t = s % T;
        double v = 0.0;
        if (T > 2) {
            if (t == 0) v = (vel[e + 6] - vel[e]) / dt;
            else if (t == T - 1) v = (vel[e] - vel[e - 6]) / dt;
            else v = (vel[e + 6] - vel[e - 6]) / (2 * dt);
        }
        acc[e] = v;
    }
}
#endif

#if defined(__HIPCC__) && defined(FBR_KERNELS_GROUPS)
// ------------------------------------------------------------------------------------------------
// Regressor WRITER of the TSQR, one lane per sample, kinematics fused in (no records): the chunks the level-0 folds read, written
// COLUMN-major -- element (chunk row o, column c) at A[c * ld + o] with o = slot * Sslot + sample -- so that the 64 samples of a wave
// are 64 consecutive doubles of one column: every store instruction writes 512 contiguous bytes (four whole lines).  It replaces the
// pair fbr_kin_kernel (9.5 KB of records per WALK-MAN sample, partially written lines) + fbr_regressor_groups_kernel (one workgroup
// per sample, ~600 instructions per thread and sample, 8-byte stores at the chunks' row stride): 4.2 + 11.7 ms per 1 M samples.
// What a column writes is resolved on the host into DESTINATIONS (chunk address of sample 0 of the row's slot in the column's position,
// 0: the row's group does not hold the column / the row is switched off), in the order the lane produces the values -- no per-entry decode:
//   colrec[c] = {first destination, number of explicit zeros};  dst[first ..]: [fb base-wrench rows][one per joint of the link's path, root
//   first][the explicit zeros: rows of the groups that hold the column but are not on the link's path, right of their first supported tile]
//   friction column: [its joint's row][zeros];  pseudo-column `cols`: per regressor row its k rhs destinations.
// The tables are read through the scalar cache (constant address space, wave-uniform addresses).  The first version of this kernel decoded
// (row, kind, level, position) entries with per-entry table lookups behind vector loads: 1350 cycles per entry; with scalar loads but a
// level-indexed branch ladder per entry: 650.
// lcol10[10 l + p]: the column of parameter p of link l (-1: not identified / not selected).  Row weights are applied here.
// ------------------------------------------------------------------------------------------------
// A workgroup = nparts waves sharing one block of 64 samples (their states are staged once): wave w walks part w of the tree.
template <int MAXD>
__global__ __launch_bounds__(64 * FBR_KINWRITE_PARTS, MAXD <= 10 ? 2 : 1) void fbr_kinwrite_kernel(DevModel m, DevKinId p, DevKinWrite wr, long S, const double *__restrict__ q,
                                                          const double *__restrict__ dq, const double *__restrict__ ddq, const double *__restrict__ bv,
                                                          const double *__restrict__ ba, const double *__restrict__ rpy, const double *__restrict__ sign,
                                                          const double *__restrict__ rhs, const double *__restrict__ wts, double *__restrict__ scratch)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x & 63, part = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nth = blockDim.x, tid = threadIdx.x;
    const int n = m.n, ldn = p.ldn, ldw = m.rows | 1;
    double *sq = smem, *sdq = sq + 64 * ldn, *sddq = sdq + 64 * ldn, *sw = sddq + 64 * ldn;  // sw: [64][ldw] row weights (has_w)
    double *scr = scratch + ((long)blockIdx.x * wr.nparts + part) * p.nslots * FBR_LINK_REC * 64 + lane;
    const long nblk = (S + 63) >> 6;
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long base = blk << 6;
        const int valid = (int)min(64L, S - base);
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
            if (wr.has_w) {
                const int rows = m.rows, cw = valid * rows;
                int wr_ = tid / rows, wc = tid - wr_ * rows;
                const int es = nth / rows, ed = nth - es * rows;
                for (int i = tid; i < cw; i += nth) {
                    sw[wr_ * ldw + wc] = wts[base * rows + i];
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
        const double *mysq = sq + ls * ldn, *mysdq = sdq + ls * ldn, *mysddq = sddq + ls * ldn, *myw = sw + ls * ldw;
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
        const fbr_clong_ptr cdst = (fbr_clong_ptr)(unsigned long)wr.dst;
        const fbr_cint_ptr crec = (fbr_cint_ptr)(unsigned long)wr.colrec, ccol = (fbr_cint_ptr)(unsigned long)(wr.lcol10 + (long)part * 10 * m.L);
        // one value: to its destination (sample 0 of the chunk) + s; the lanes of a wave write 64 consecutive doubles
        const unsigned sbyte = (unsigned)s << 3;  // (s: sample index inside the chunk -- one launch per chunk; a chunk's column is far below 4 GB)
        auto put = [&](long d0, double v) {
            if (d0 != 0 && live) __builtin_nontemporal_store(v, (fbr_gdouble_ptr)((fbr_gchar_ptr)d0 + sbyte));  // scalar base + 32-bit lane offset
        };
        auto link = [&](int l, int depth, const double *rec, const double (*Sst)[6], const int *lvd, double *F) {
            (void)F;
            // the vector loads of the step are waited for here, once: the stores below share their counter, and behind the branches of the
            // column code the compiler would otherwise wait for counter 0 -- the store before -- at every store (see fbr_gram64.h)
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
#pragma unroll
            for (int pp = 0; pp < 10; pp++) {
                const int c = ccol[10 * l + pp];
                if (c < 0) continue;
                const int d0 = crec[2 * c], nz = crec[2 * c + 1];
                if (d0 < 0) continue;  // (the column is not factorised)
                // the record's destinations are requested TOGETHER, before anything is computed (one round trip to the scalar cache / L2 per
                // column instead of one per value; reads past the record's end stay inside the padded table and are never used)
                long db[6], dj[MAXD];
#pragma unroll
                for (int i = 0; i < 6; i++) db[i] = cdst[d0 + i];
#pragma unroll
                for (int j = 0; j < MAXD; j++) dj[j] = cdst[d0 + m.fb + j];
                double w6[6];
                fbr_unit_wrench(rec, pp, w6);
#pragma unroll
                for (int i = 0; i < 6; i++)
                    if (i < m.fb) put(db[i], wr.has_w ? w6[i] * myw[i] : w6[i]);
#pragma unroll
                for (int j = 0; j < MAXD; j++)
                    if (j < depth) {
                        const double v = fbr_dot6(Sst[j], w6);
                        put(dj[j], wr.has_w ? v * myw[m.fb + lvd[j]] : v);
                    }
                for (int z = 0; z < nz; z++) put(cdst[d0 + m.fb + depth + z], 0.0);
            }
        };
        auto emit = [&](int, double) {};
        fbr_kinid_lane<MAXD, false>(wr.part_nsteps[part], p.maxlvl, p.steps + wr.part_step0[part] * FBR_KINID_STEP, p.endflush, m.floating, m.g, m.fb,
                                    state, basest, save, load, link, emit, consts);
        if (part != wr.nparts - 1) continue;  // (friction and rhs columns: the last part, which the cut leaves the lightest)
        // friction columns: one value on the row of the column's joint, explicit zeros on the other rows of the groups that hold it
        for (int c = wr.ninert; c < wr.cols; c++) {
            const int d0 = crec[2 * c], nz = crec[2 * c + 1];
            if (d0 < 0) continue;
            const int4 cd = m.coldesc[c];
            const double fv = fbr_friction_value(cd.z, mysdq[cd.w], sign ? sign[s * n + cd.w] : 0.0, m.stribeck);
            put(cdst[d0], wr.has_w ? fv * myw[m.fb + cd.w] : fv);
            for (int z = 0; z < nz; z++) put(cdst[d0 + 1 + z], 0.0);
        }
        // rhs columns: k destinations per regressor row
        {
            const int d0 = crec[2 * wr.cols];
            for (int r = 0; r < m.rows; r++)
                for (int i = 0; i < wr.k; i++) {
                    const double v = rhs[(s * m.rows + r) * wr.k + i];
                    put(cdst[d0 + r * wr.k + i], wr.has_w ? v * myw[r] : v);
                }
        }
    }
}
#endif
