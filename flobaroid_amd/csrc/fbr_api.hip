// fbr_api.hip -- C-ABI of libfbr (see include/fbr.h): model handle, options, state staging, per-sample entry points.
// gfx950 only; there is deliberately no CPU path in this library.  The fused Gram lives in fbr_gram_api.hip, the TSQR in
// fbr_tsqr_api.hip, the signal conditioning in fbr_signal_api.hip, the collision sets and their calls in fbr_collision_api.hip.
#define FBR_KERNELS_CORE
#include "fbr_internal.h"
#include "fbr_reduce.h"

thread_local std::string g_fbr_err;

// ------------------------------------------------------------------------------------------------
// 101 (round 6): fbr_topology.joint_type, the num_samples argument of fbr_gram_program_info / fbr_model_link_merge_info (both added in
// round 5 under 100), option "fused_id"; 102: fbr_gram_lane_info, options "gram_lane" / "gram_force_tiles" / "tsqr_force_group"; 103: fbr_candidate_extrema;
// 104: fbr_model_set_capsules, fbr_candidate_capsule_distances (and, under the same number, fbr_regressor_weights, fbr_fourier_gradient,
// fbr_capsule_distance_gradients, fbr_fourier_position_chain, fbr_torque_row_sweep, fbr_fourier_state_chain, fbr_suspended_base_motion,
// fbr_suspended_records, fbr_model_set_boxes, fbr_candidate_box_distances, fbr_box_distance_gradients, fbr_model_set_hulls, fbr_candidate_hull_distances,
// fbr_hull_distance_gradients, fbr_model_set_hull_meshes, fbr_mesh_distance_gradients: added symbols change no signature, and _lib.py names a library
// that lacks one).
// flobaroid_amd/_lib.py refuses a library of another version than the header it was written for.
extern "C" int fbr_version(void) { return FBR_VERSION; }

// (dispatched once on each of a model's two Gram streams at creation: see create_model)
__global__ void fbr_noop_kernel() {}

// The HIP runtime does not survive fork(): a child that inherits an initialised runtime hangs or fails in its first call.  The
// reference's multi-process users build one Model per worker AFTER the fork (analyticalGradient.py:188-210); this records the process
// that first touched HIP through the library so that the other order is reported instead of deadlocking.
static pid_t g_hip_pid = 0;
static bool forked_after_hip_init()
{
    const pid_t me = getpid();
    if (g_hip_pid == 0) g_hip_pid = me;
    if (g_hip_pid == me) return false;
    set_err("HIP was initialised in the parent process before fork(): create the model in the worker (after the fork) or start "
            "workers with the 'spawn' method");
    return true;
}
int enter(fbr_model *m)
{
    if (m->pid != getpid()) {
        set_err("this fbr_model was created in another process (before fork()): create one per process");
        return FBR_E_FORK;
    }
    HIPCHK(hipSetDevice(m->device));
    return FBR_OK;
}

// entry of a blocking call that does not go through stage_states: every asynchronous submission before it has completed
int enter_blocking(fbr_model *m)
{
    if (int rc = enter(m)) return rc;
    return wait_ticket(m, m->next_ticket - 1);
}

extern "C" int fbr_device_count(void)
{
    if (forked_after_hip_init()) return 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char *fbr_last_error(void) { return g_fbr_err.c_str(); }

static int build_reduction(fbr_model *m, const fbr_topology *t, int which);
static int create_model(const fbr_topology *t, int device, fbr_model **out, bool allow_merge, const unsigned short *linkmask = nullptr)  // (t->joint_type: NULL or [L])
{
    if (!t || !out) {
        set_err("null argument");
        return FBR_E_INVALID;
    }
    *out = nullptr;
    if (forked_after_hip_init()) return FBR_E_FORK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_err("no HIP device available (libfbr has no CPU fallback)");
        return FBR_E_NODEVICE;
    }
    if (device < 0 || device >= ndev) {
        set_err("device index out of range");
        return FBR_E_INVALID;
    }
    std::unique_ptr<fbr_model> m(new fbr_model());
    try {
        m->hm.build(t->num_links, t->num_dofs, t->parent, t->dof_index, t->rest_R, t->rest_p, t->axis, t->floating_base,
                    t->gravity, t->friction, t->friction_symmetric, t->gravity_only, t->stribeck_velocity, linkmask, t->joint_type);
    } catch (const std::exception &e) {
        set_err(std::string("invalid topology: ") + e.what());
        return FBR_E_INVALID;
    }
    m->device = device;
    m->pid = getpid();
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    m->num_cus = prop.multiProcessorCount;
    HIPCHK(hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking));
    m->stream = m->own_stream;
    {
        // The producer stream must not share a hardware queue with the stream the Gram kernel runs on, or the two serialise
        // (seen under torch.distributed, where RCCL's streams shift HIP's round-robin stream -> queue assignment).  A stream of
        // another priority level gets a queue of its own; the producer is the background work, so it takes the lowest.
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(hipStreamCreateWithPriority(&m->side, hipStreamNonBlocking, least));
        // HIP binds a stream to a hardware queue at its first dispatch: both streams of the Gram pass dispatch once HERE, so that their queues do not
        // depend on which other streams (TSQR trees, copies, the caller's) were used first -- seen in bench.py, round 6: the grouped Gram after a
        // masked TSQR call 13.3 instead of 5.2 ms when the producer stream's first kernel came after the TSQR's side streams'
        hipLaunchKernelGGL(fbr_noop_kernel, dim3(1), dim3(64), 0, m->own_stream);
        hipLaunchKernelGGL(fbr_noop_kernel, dim3(1), dim3(64), 0, m->side);
        HIPCHK(hipGetLastError());
    }
    for (int i = 0; i < 2; i++) {
        HIPCHK(hipEventCreateWithFlags(&m->ev_done[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&m->ev_h2d[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&m->ev_pack[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&m->ev_gram[i], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m->ev_tsqr_l0, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m->ev_tsqr_pro, hipEventDisableTiming));
    HIPCHK(hipMalloc((void **)&m->tsqr_err, sizeof(unsigned)));
    HIPCHK(hipMemset(m->tsqr_err, 0, sizeof(unsigned)));
    HIPCHK(hipHostMalloc((void **)&m->tsqr_err_host, 2 * sizeof(unsigned), hipHostMallocDefault));
    m->tsqr_err_host[0] = m->tsqr_err_host[1] = 0;

    const FbrHostModel &hm = m->hm;
    DevModel &dm = m->dm;
    memset(&dm, 0, sizeof(dm));
    dm.L = hm.L; dm.n = hm.n; dm.fb = hm.fb; dm.rows = hm.rows; dm.cols = hm.cols; dm.cpl = hm.cpl;
    dm.floating = hm.floating; dm.rec = hm.rec_size(); dm.maxd = std::max(hm.maxdepth, 1);
    dm.nw = std::max(1, (hm.n + 31) / 32);
    dm.fric = hm.fric; dm.grav_only = hm.grav_only; dm.fstart = hm.friction_start();
    for (int i = 0; i < 3; i++) dm.g[i] = hm.gravity[i];
    dm.stribeck = hm.stribeck;
    std::vector<int> pathlen(hm.L), pathtab((size_t)hm.L * dm.maxd, 0), pathpos((size_t)hm.L * dm.maxd, 0);
    std::vector<unsigned> anc((size_t)hm.L * dm.nw, 0u);
    std::vector<std::vector<int>> sub(std::max(hm.n, 1));
    std::vector<int> dof_link(std::max(hm.n, 1), 0);
    for (int l = 0; l < hm.L; l++) {
        pathlen[l] = (int)hm.path[l].size();
        for (size_t j = 0; j < hm.path[l].size(); j++) {
            int d = hm.path[l][j];
            pathtab[(size_t)l * dm.maxd + j] = d;
            pathpos[(size_t)l * dm.maxd + j] = hm.ppos[l][j];
            anc[(size_t)l * dm.nw + (d >> 5)] |= 1u << (d & 31);
            sub[d].push_back(l);
        }
        if (hm.dof[l] >= 0) dof_link[hm.dof[l]] = l;
    }
    std::vector<int> sub_begin(hm.n + 1, 0), sub_links;
    for (int d = 0; d < hm.n; d++) {
        sub_begin[d] = (int)sub_links.size();
        sub_links.insert(sub_links.end(), sub[d].begin(), sub[d].end());
    }
    sub_begin[hm.n] = (int)sub_links.size();
    std::vector<int4> cd(hm.cols);
    for (int c = 0; c < hm.cols; c++) cd[c] = make_int4(hm.coldesc[c].kind, hm.coldesc[c].link, hm.coldesc[c].pidx, hm.coldesc[c].joint);
    int rc = 0;
    m->tables.reserve(32);
    if ((rc = upload(m->tables, hm.order, &dm.order))) return rc;
    if ((rc = upload(m->tables, hm.parent, &dm.parent))) return rc;
    if ((rc = upload(m->tables, hm.dof, &dm.dof))) return rc;
    if ((rc = upload(m->tables, hm.jtype, &dm.jtype))) return rc;
    if ((rc = upload(m->tables, hm.restR, &dm.restR))) return rc;
    if ((rc = upload(m->tables, hm.restp, &dm.restp))) return rc;
    if ((rc = upload(m->tables, hm.axis, &dm.axis))) return rc;
    if ((rc = upload(m->tables, pathlen, &dm.pathlen))) return rc;
    if ((rc = upload(m->tables, pathtab, &dm.pathtab))) return rc;
    if ((rc = upload(m->tables, pathpos, &dm.pathpos))) return rc;
    if ((rc = upload(m->tables, anc, &dm.ancmask))) return rc;
    if ((rc = upload(m->tables, cd, &dm.coldesc))) return rc;
    if ((rc = upload(m->tables, sub_begin, &dm.sub_begin))) return rc;
    if ((rc = upload(m->tables, sub_links, &dm.sub_links))) return rc;
    if ((rc = upload(m->tables, dof_link, &dm.dof_link))) return rc;
    if (hm.maxdepth <= FBR_KINID_MAXD) {
        try {
            fbr_kinid_build(hm, m->kinid);
        } catch (const std::exception &e) {
            set_err(std::string("internal: ") + e.what());
            return FBR_E_INVALID;
        }
        if ((rc = upload(m->tables, m->kinid.steps, &m->kinid_steps))) return rc;
        if ((rc = upload(m->tables, m->kinid.endflush, &m->kinid_endflush))) return rc;
    }
    if (allow_merge) {  // (always built; the options "link_merge" / "regroup" decide per call whether they are used)
        if ((rc = build_reduction(m.get(), t, 0))) return rc;
        if ((rc = build_reduction(m.get(), t, 1))) return rc;
    }
    *out = m.release();
    return FBR_OK;
}

extern "C" int fbr_model_create(const fbr_topology *t, int device, fbr_model **out) { return create_model(t, device, out, true); }

// ------------------------------------------------------------------------------------------------
// Column reductions (fbr_reduce.h has the mathematics: fixed links merged into the bodies they ride on, revolute links regrouped, and the
// constant matrix E with [Y | rhs] = [Y_red | rhs] E).  The reductions run on the REDUCED robot and are expanded at the end of the call:
// G = E^T G_red E,  R = qr(R_red E).  which = 0: merged (m->rdm[0]); which = 1: merged + regrouped (column masks, m->rdm[1]).
// ------------------------------------------------------------------------------------------------
static int build_reduction(fbr_model *m, const fbr_topology *t, int which)
{
    FbrReducedRobot rr;
    if (!fbr_reduce_robot(m->hm, which, rr)) return FBR_OK;
    fbr_topology tr = *t;
    tr.num_links = rr.Lr;
    tr.parent = rr.parent.data();
    tr.dof_index = rr.dof.data();
    tr.rest_R = rr.restR.data();
    tr.rest_p = rr.restp.data();
    tr.axis = rr.axis.data();
    tr.joint_type = rr.jtype.data();
    fbr_model *red = nullptr;
    if (int rc = create_model(&tr, m->device, &red, false, rr.masked ? rr.masks.data() : nullptr)) return rc;
    m->rdm[which].reset(red);
    red->is_reduction = true;
    std::vector<int> beg, row;
    std::vector<double> val;
    fbr_reduction_matrix(m->hm, rr, red->hm, beg, row, val);
    int rc;
    if ((rc = upload(m->tables, beg, &m->E_beg[which])) || (rc = upload(m->tables, row, &m->E_row[which])) ||
        (rc = upload(m->tables, val, &m->E_val[which])))
        return rc;
    m->hE_beg[which] = beg;
    m->hE_row[which] = row;
    m->hE_val[which] = val;
    return FBR_OK;
}
extern "C" void fbr_model_destroy(fbr_model *m)
{
    if (m && m->pid != getpid()) return;  // a handle inherited through fork(): its device resources belong to the parent, nothing to free here
    delete m;  // ~fbr_model releases the device memory, streams and events
}

// the reduced model a fused Gram pass runs on (-1: the model itself)
int pick_gram_reduction(const fbr_model *m, long S)
{
    const FbrOptions &o = m->opt;
    if (!o.link_merge) return -1;
    // S >= 0: a call over S samples.  The reduced pass costs a second model's launches and two expansion kernels (~0.15 ms): small
    // robots on short batches are faster over all their columns (KUKA, 80 -> 59 columns, 50 k samples: 0.73 against 0.82 ... 1.08 ms)
    if (S >= 0) {
        // (against the reduction that would be taken: the regrouped model within the fused kernel's 60 rows, else the merged one)
        const bool regrouped = m->rdm[1] && o.regroup && (m->hm.rows + 3) / 4 * 4 <= 60;
        const fbr_model *r = regrouped ? m->rdm[1].get() : m->rdm[0].get();
        if (r && (double)S * (m->hm.cols - r->hm.cols) * m->hm.cols < o.reduce_min_work) return -1;
    }
    // (robots beyond the fused kernel's 60 rows take their Gram from a TSQR factor, gram_via_tsqr: every path of the merged model)
    if (m->rdm[1] && o.regroup && (m->hm.rows + 3) / 4 * 4 <= 60) return 1;
    return m->rdm[0] ? 0 : -1;
}

extern "C" int fbr_model_link_merge_info(const fbr_model *m, int64_t num_samples, int32_t *moving_links, int32_t *reduced_cols)
{
    if (!m) {
        set_err("null model");
        return FBR_E_INVALID;
    }
    const int w = pick_gram_reduction(m, num_samples < 0 ? -1 : (long)num_samples);
    if (moving_links) *moving_links = w >= 0 ? m->rdm[w]->hm.L : m->hm.L;
    if (reduced_cols) *reduced_cols = w >= 0 ? m->rdm[w]->hm.cols : m->hm.cols;
    return FBR_OK;
}

static void clear_programs(fbr_model *m)
{
    m->gram.clear();  // (Gram programs and their device tables are rebuilt on the next call)
}

extern "C" int fbr_model_set_option(fbr_model *m, const char *key, double value)
{
    const FbrOptionKey *k = fbr_option_find(key);
    if (!m || !k || !(value == value)) {
        set_err(std::string("fbr_model_set_option: unknown option '") + (key ? key : "(null)") + "' or bad value");
        return FBR_E_INVALID;
    }
    if (m->opt.*(k->field) == value) return FBR_OK;
    // nothing may be in flight when the behaviour of the calls changes (tile programs are freed, chunk sizes move)
    if (int rc = enter_blocking(m)) return rc;
    HIPCHK(hipStreamSynchronize(m->stream));
    m->opt.*(k->field) = value;
    for (auto &r : m->rdm)
        if (r) r->opt = m->opt;
    if (k->rebuild_programs) {
        clear_programs(m);
        for (auto &r : m->rdm)
            if (r) clear_programs(r.get());
    }
    m->rd_grouped = -1;
    return FBR_OK;
}

extern "C" int fbr_model_get_option(const fbr_model *m, const char *key, double *value)
{
    const FbrOptionKey *k = fbr_option_find(key);
    if (!m || !k || !value) {
        set_err(std::string("fbr_model_get_option: unknown option '") + (key ? key : "(null)") + "'");
        return FBR_E_INVALID;
    }
    *value = m->opt.*(k->field);
    return FBR_OK;
}

extern "C" int fbr_model_option_name(int32_t index, const char **name)
{
    int n = 0;
    const FbrOptionKey *k = fbr_option_keys(&n);
    if (!name || index < 0 || index >= n) return FBR_E_INVALID;  // (index == count: the end of the list)
    *name = k[index].name;
    return FBR_OK;
}

extern "C" int fbr_model_dims(const fbr_model *m, int32_t *rows, int32_t *cols)
{
    if (!m) {
        set_err("null model");
        return FBR_E_INVALID;
    }
    if (rows) *rows = m->hm.rows;
    if (cols) *cols = m->hm.cols;
    return FBR_OK;
}

extern "C" int fbr_model_set_stream(fbr_model *m, void *s)
{
    if (!m) {
        set_err("null model");
        return FBR_E_INVALID;
    }
    // submissions in flight were enqueued on the stream used so far (their completion events and Gram launches live there): they
    // are waited for before the switch, so that fbr_wait / the destructor never look at a stream that does not carry them
    const hipStream_t next = s ? (hipStream_t)s : m->own_stream;
    if (next != m->stream) {
        if (int rc = enter_blocking(m)) return rc;
    }
    m->stream = next;
    for (auto &r : m->rdm)
        if (r) r->stream = next;  // (their submissions were waited for through this model's tickets)
    return FBR_OK;
}

extern "C" int fbr_profile_enable(fbr_model *m, int32_t on)
{
    if (!m) {
        set_err("null model");
        return FBR_E_INVALID;
    }
    m->prof = on != 0;
    for (auto &r : m->rdm)
        if (r) r->prof = m->prof;
    return FBR_OK;
}

extern "C" int fbr_profile_get(fbr_model *m, double *ms_out, int64_t *launches_out)
{
    if (!m) {
        set_err("null model");
        return FBR_E_INVALID;
    }
    for (int i = 0; i < FBR_PROF_COUNT; i++) {
        for (auto &r : m->rdm)
            if (r) {  // (the passes that ran on the reduced models)
                m->prof_ms[i] += r->prof_ms[i];
                m->prof_n[i] += r->prof_n[i];
                r->prof_ms[i] = 0;
                r->prof_n[i] = 0;
            }
        if (ms_out) ms_out[i] = m->prof_ms[i];
        if (launches_out) launches_out[i] = m->prof_n[i];
        m->prof_ms[i] = 0;
        m->prof_n[i] = 0;
    }
    return FBR_OK;
}
int stage_one(fbr_model *m, DevBuf &buf, const double *src, size_t count, int mem, const double **dst)
{
    if (!src) {
        *dst = nullptr;
        return FBR_OK;
    }
    if (mem == FBR_DEVICE) {
        *dst = src;
        return FBR_OK;
    }
    int rc = buf.ensure(std::max<size_t>(count, 1) * sizeof(double));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(buf.p, src, count * sizeof(double), hipMemcpyHostToDevice, m->stream));
    *dst = (const double *)buf.p;
    return FBR_OK;
}

// true iff p is pinned (page-locked / registered) host memory: hipMemcpyAsync from it is asynchronous
bool is_pinned_host(const void *p)
{
    if (!p) return true;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// defer_host: leave HOST inputs where they are (d receives the host pointers): the caller stages them chunk by chunk
int stage_states(fbr_model *m, const fbr_states *st, DevStates *d, bool need_vel, bool defer_host)
{
    if (!m || !st) {
        set_err("null argument");
        return FBR_E_INVALID;
    }
    if (st->num_samples < 0 || (st->mem != FBR_HOST && st->mem != FBR_DEVICE)) {
        set_err("bad fbr_states header");
        return FBR_E_INVALID;
    }
    const FbrHostModel &hm = m->hm;
    if (!st->q || (need_vel && (!st->dq || !st->ddq))) {
        set_err("q/dq/ddq must not be NULL");
        return FBR_E_INVALID;
    }
    if (hm.floating && (!st->base_rpy || (need_vel && (!st->base_vel || !st->base_acc)))) {
        set_err("floating base model needs base_vel/base_acc/base_rpy");
        return FBR_E_INVALID;
    }
    if (need_vel && hm.fric && !st->sign) {
        set_err("friction layout needs the Coulomb sign series (fbr_states.sign)");
        return FBR_E_INVALID;
    }
    if (int rc_enter = enter(m)) return rc_enter;
    if (!m->submitting) {  // blocking entry points run after every asynchronous submission before them
        if (int rc_w = wait_ticket(m, m->next_ticket - 1)) return rc_w;
    }
    const size_t S = (size_t)st->num_samples;
    d->S = (long)S;
    int rc;
    if (defer_host && st->mem == FBR_HOST) {
        d->q = st->q;
        d->dq = st->dq;
        d->ddq = st->ddq;
        d->rpy = hm.floating ? st->base_rpy : nullptr;
        d->bv = hm.floating ? st->base_vel : nullptr;
        d->ba = hm.floating ? st->base_acc : nullptr;
        d->sign = hm.fric ? st->sign : nullptr;
        return FBR_OK;
    }
    if ((rc = stage_one(m, m->st_q, st->q, S * hm.n, st->mem, &d->q))) return rc;
    if ((rc = stage_one(m, m->st_dq, st->dq ? st->dq : st->q, S * hm.n, st->mem, &d->dq))) return rc;
    if ((rc = stage_one(m, m->st_ddq, st->ddq ? st->ddq : st->q, S * hm.n, st->mem, &d->ddq))) return rc;
    if (hm.floating) {
        if ((rc = stage_one(m, m->st_rpy, st->base_rpy, S * 3, st->mem, &d->rpy))) return rc;
        // without velocities (contact Jacobian only) the twist inputs are irrelevant: reuse any valid buffer
        if ((rc = stage_one(m, m->st_bv, st->base_vel, S * 6, st->mem, &d->bv))) return rc;
        if ((rc = stage_one(m, m->st_ba, st->base_acc, S * 6, st->mem, &d->ba))) return rc;
    }
    if (hm.fric && st->sign)
        if ((rc = stage_one(m, m->st_sign, st->sign, S * hm.n, st->mem, &d->sign))) return rc;
    return FBR_OK;
}

long chunk_size(const fbr_model *m, long S)
{
    const size_t per = (size_t)m->hm.rec_size() * sizeof(double);
    long ch = (long)((size_t)(768u << 20) / per);
    if (ch < 1024) ch = 1024;
    if (m->opt.chunk_samples >= 1) ch = (long)m->opt.chunk_samples;  // tests: force the multi-chunk paths at small sizes
    return std::min(S, ch);
}

int run_kin(fbr_model *m, const DevStates &d, long s0, long cs, hipStream_t st, DevBuf *recbuf)
{
    const FbrHostModel &hm = m->hm;
    if (!st) st = m->stream;
    if (!recbuf) recbuf = &m->rec;
    int rc = recbuf->ensure((size_t)cs * hm.rec_size() * sizeof(double));
    if (rc) return rc;
    const int threads = 256;
    const int blocks = (int)((cs + threads - 1) / threads);
    ProfScope ps(m, FBR_PROF_KIN, st);
    // (one instance, no register cap: the 96-VGPR instance that once ran beside the Gram kernel spilled 41 registers and, since the column
    // reductions, was the slower one there as well -- kin 6.2 instead of 5.3 ms per 1 M samples: DESIGN.md 10)
    hipLaunchKernelGGL(fbr_kin_kernel<2>, dim3(blocks), dim3(threads), 0, st, m->dm, cs, d.q + s0 * hm.n, d.dq + s0 * hm.n, d.ddq + s0 * hm.n,
                       d.bv ? d.bv + s0 * 6 : nullptr, d.ba ? d.ba + s0 * 6 : nullptr, d.rpy ? d.rpy + s0 * 3 : nullptr, recbuf->as<double>());
    HIPCHK(hipGetLastError());
    return FBR_OK;
}

int finish_output(fbr_model *m, double *dev_src, double *user_dst, size_t count, int out_mem)
{
    if (out_mem == FBR_HOST)
        HIPCHK(hipMemcpyAsync(user_dst, dev_src, count * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    prof_collect(m);
    return FBR_OK;
}

// ------------------------------------------------------------------------------------------------
int launch_regressor(fbr_model *m, const DevStates &d, long s0, long cs, double *dst, int ldy, long rs_s, long rs_r, const int *linkpos, const int *skipfc)
{
    const FbrHostModel &hm = m->hm;
    const size_t lds = (size_t)hm.rec_size() * sizeof(double);
    const int spb = std::max(1, std::min(16, 256 / std::max(1, hm.cols / 2)));  // samples side by side in one workgroup
    const size_t lds2 = lds * spb;
    ProfScope ps(m, FBR_PROF_REGRESSOR);
    // even column count (and a 16-byte aligned output): paired columns, 16-byte stores
    if ((hm.cols & 1) == 0 && (((uintptr_t)dst) & 15) == 0 && (ldy & 1) == 0) {
        HIPCHK(hipFuncSetAttribute((const void *)fbr_regressor2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
        hipLaunchKernelGGL(fbr_regressor2_kernel, dim3((unsigned)std::min<long>((cs + spb - 1) / spb, (long)m->num_cus * 8)), dim3(256), lds2, m->stream, m->dm, cs, spb,
                           m->rec.as<double>(), d.dq + s0 * hm.n, d.sign ? d.sign + s0 * hm.n : nullptr, dst, ldy, rs_s, rs_r, linkpos, skipfc);
    } else {
        HIPCHK(hipFuncSetAttribute((const void *)fbr_regressor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(fbr_regressor_kernel, dim3((unsigned)std::min<long>(cs, (long)m->num_cus * 8)), dim3(256), lds, m->stream, m->dm, cs, m->rec.as<double>(),
                           d.dq + s0 * hm.n, d.sign ? d.sign + s0 * hm.n : nullptr, dst, ldy, rs_s, rs_r, linkpos, skipfc);
    }
    HIPCHK(hipGetLastError());
    return FBR_OK;
}

extern "C" int fbr_regressor_batch(fbr_model *m, const fbr_states *st, double *Y_out, int32_t out_mem)
{
    DevStates d;
    int rc = stage_states(m, st, &d);
    if (rc) return rc;
    if (!Y_out) {
        set_err("Y_out is NULL");
        return FBR_E_INVALID;
    }
    const FbrHostModel &hm = m->hm;
    const size_t per = (size_t)hm.rows * hm.cols;
    const long S = d.S;
    if (S == 0) return FBR_OK;
    long ch = chunk_size(m, S);
    if (out_mem == FBR_HOST) {
        // bound the device staging buffer of the output to ~1 GiB
        long och = (long)((size_t)(1u << 30) / (per * sizeof(double)));
        ch = std::max(1L, std::min(ch, och));
        if ((rc = m->out_tmp.ensure((size_t)ch * per * sizeof(double)))) return rc;
    }
    for (long s0 = 0; s0 < S; s0 += ch) {
        const long cs = std::min(ch, S - s0);
        if ((rc = run_kin(m, d, s0, cs))) return rc;
        double *dst = (out_mem == FBR_HOST) ? m->out_tmp.as<double>() : Y_out + (size_t)s0 * per;
        if ((rc = launch_regressor(m, d, s0, cs, dst, hm.cols, (long)hm.rows, 1L, nullptr, nullptr))) return rc;
        if (out_mem == FBR_HOST) {
            HIPCHK(hipMemcpyAsync(Y_out + (size_t)s0 * per, dst, (size_t)cs * per * sizeof(double), hipMemcpyDeviceToHost,
                                  m->stream));
            HIPCHK(hipStreamSynchronize(m->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    prof_collect(m);
    return FBR_OK;
}

// dynamic LDS of fbr_kinid_kernel: q, dq and ddq of a block of 64 samples
static size_t kinid_lds(const fbr_model *m) { return (size_t)3 * 64 * (std::max(m->hm.n, 1) | 1) * sizeof(double); }
// the fused kernel serves this model: a program exists (joint paths of at most FBR_KINID_MAXD) and the staged states fit a workgroup's
// 160 KiB of LDS (up to 105 DOF); otherwise the two-kernel path (run_kin + fbr_id_kernel / fbr_contact_kernel)
static bool kinid_fits(const fbr_model *m) { return m->opt.fused_id != 0 && m->kinid.nsteps > 0 && kinid_lds(m) <= (size_t)160 * 1024; }
// Fused kinematics + torques (csrc/fbr_kinid.h): one kernel, one lane per sample, the link records stay in registers, branch-point
// records in a per-wave scratch.  mode 0 / 1: x = parameters (device); mode 2: x = [S][6] contact wrenches at frame (flink, fp).
// ex (mode 0 only): the candidate-extrema instance, which writes the partials of ex instead of dst.
static int launch_kinid(fbr_model *m, const DevStates &d, long S, const double *dvs, const double *x, int mode, double *dst, int flink, const double *fp,
                        const DevKinExt *ex = nullptr)
{
    const DevKinId kp = kinid_params(m);
    const size_t lds = kinid_lds(m);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (size_t)(150 << 10) / std::max<size_t>(lds, 1)));
    const long nblk = ex ? ex->nblk : (S + 63) / 64;
    const int blocks = (int)std::min<long>(nblk, (long)m->num_cus * per_cu);
    if (int rc = m->kinid_scratch.ensure((size_t)blocks * std::max(kp.nslots, 1) * FBR_LINK_REC * 64 * sizeof(double))) return rc;
    const double f0 = fp ? fp[0] : 0.0, f1 = fp ? fp[1] : 0.0, f2 = fp ? fp[2] : 0.0;
    const DevKinExt ex0 = ex ? *ex : DevKinExt{0, 0, 0, nullptr, nullptr};
    ProfScope ps(m, FBR_PROF_ID);
    return fbr_by_depth<4, 8, 12, FBR_KINID_MAXD>(kp.maxlvl, [&](auto D) -> int {
        const auto kern = ex ? fbr_kinid_kernel<D, true> : fbr_kinid_kernel<D, false>;
        HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, m->stream, m->dm, kp, S, d.q, d.dq, d.ddq, d.bv, d.ba, d.rpy, d.sign,
                           dvs, x, mode, dst, m->kinid_scratch.as<double>(), flink, f0, f1, f2, ex0);
        HIPCHK(hipGetLastError());
        return FBR_OK;
    });
}

// fbr_candidate_extrema's request to run_id: the torques are reduced to per-candidate extrema instead of returned
struct ExtremaReq {
    long ncand;
    double *val_out;
    int64_t *idx_out;
};

// the tiles of ncand candidates of S / ncand samples each, their partials in m->ext_part
static int extrema_tiles(fbr_model *m, long S, long ncand, DevKinExt *ex)
{
    const long T = S / ncand, tiles = (T + 63) / 64;
    const size_t cnt = (size_t)ncand * tiles * 4 * std::max(m->hm.n, 1);
    if (int rc = m->ext_part.ensure(cnt * (sizeof(double) + sizeof(long)))) return rc;
    *ex = DevKinExt{T, tiles, ncand * tiles, m->ext_part.as<double>(), (long *)(m->ext_part.as<double>() + cnt)};
    return FBR_OK;
}

// the candidates' partials reduced in tile order into [ncand][4][n] values and indices (the caller's memory space)
static int finish_extrema(fbr_model *m, const DevKinExt &ex, const ExtremaReq &rq, int32_t out_mem)
{
    const int n = m->hm.n;
    const size_t cnt = (size_t)rq.ncand * 4 * n;
    double *val = rq.val_out;
    long *idx = (long *)rq.idx_out;
    if (out_mem == FBR_HOST) {
        if (int rc = m->ext_out.ensure(cnt * (sizeof(double) + sizeof(long)))) return rc;
        val = m->ext_out.as<double>();
        idx = (long *)(val + cnt);
    }
    {
        ProfScope ps(m, FBR_PROF_ID);
        hipLaunchKernelGGL(fbr_extrema_finish_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, m->stream, ex, n, rq.ncand, val, idx);
        HIPCHK(hipGetLastError());
    }
    if (out_mem == FBR_HOST) {
        HIPCHK(hipMemcpyAsync(rq.val_out, val, cnt * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(rq.idx_out, idx, cnt * sizeof(long), hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    prof_collect(m);
    return FBR_OK;
}

// Y x = Y_red (E x): torques are linear in the parameters, and the parameters of a link welded to a moving body are parameters of that
// body (build_reduction, merged model rdm[0]: every moving link keeps its ten columns).  The kinematics and the per-link wrench loop
// then run over the moving bodies only (WALK-MAN: 30 of 48 links) -- same rows, same result to rounding.  Returns the merged model that
// serves x (on m's stream, its parameters in xr / *nxr), or nullptr: the call runs on m itself unless *rc is set.
static fbr_model *merged_for_torques(fbr_model *m, const fbr_states *st, const double *x, int nx, int mode, std::vector<double> &xr, int *nxr, int *rc)
{
    if (!(m && x && st && m->rdm[0] && m->opt.link_merge && m->pid == getpid())) return nullptr;
    fbr_model *r = m->rdm[0].get();
    const FbrHostModel &hm = m->hm, &rh = r->hm;
    const int ninert = hm.cpl * hm.L, rin = rh.cpl * rh.L;
    const int full = mode == 0 ? ninert : hm.cols;  // mode 0: the inertial block of x_std; mode 1: every identified column
    if (hm.cpl != 10 || nx < full) return nullptr;
    xr.assign((size_t)std::max(rin + (nx - ninert), rh.cols), 0.0);
    const std::vector<int> &eb = m->hE_beg[0], &er = m->hE_row[0];
    const std::vector<double> &ev = m->hE_val[0];
    for (int j = 0; j < ninert; j++)
        for (int e = eb[j]; e < eb[j + 1]; e++) xr[er[e]] += ev[e] * x[j];
    for (int j = ninert; j < nx; j++) xr[rin + (j - ninert)] = x[j];  // friction slots / columns: the same joints in the same layout
    if ((*rc = enter_blocking(m))) return nullptr;
    r->stream = m->stream;
    r->prof = m->prof;
    *nxr = rin + (nx - ninert);
    return r;
}

// the two-kernel torques of S staged samples (kinematic records through HBM, chunk by chunk): tau [S][rows] to dst (device)
static int launch_id_two_kernel(fbr_model *m, const DevStates &d, long S, const double *dvs, const double *x, int mode, double *dst)
{
    const FbrHostModel &hm = m->hm;
    // one wave per sample, each with its record and link forces in the LDS: up to four waves per workgroup, fewer for large trees
    const size_t per_wave = (size_t)(hm.rec_size() + 6 * hm.L) * sizeof(double);
    const int waves = (int)std::min<size_t>(4, (size_t)160 * 1024 / per_wave);
    if (waves < 1) {
        set_err("model too large: the inverse dynamics of one sample needs more than 160 KiB of LDS");
        return FBR_E_UNSUPPORTED;
    }
    const size_t lds = (size_t)waves * per_wave;
    HIPCHK(hipFuncSetAttribute((const void *)fbr_id_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long ch = chunk_size(m, S);
    for (long s0 = 0; s0 < S; s0 += ch) {
        const long cs = std::min(ch, S - s0);
        if (int rc = run_kin(m, d, s0, cs)) return rc;
        const int blocks = (int)std::min<long>((cs + waves - 1) / waves, (long)m->num_cus * 8);
        ProfScope ps(m, FBR_PROF_ID);
        hipLaunchKernelGGL(fbr_id_kernel, dim3(blocks), dim3(64 * waves), lds, m->stream, m->dm, cs, m->rec.as<double>(),
                           d.dq + s0 * hm.n, d.sign ? d.sign + s0 * hm.n : nullptr, dvs ? dvs + s0 * hm.n : nullptr, x, mode, dst + (size_t)s0 * hm.rows);
        HIPCHK(hipGetLastError());
    }
    return FBR_OK;
}

// ext: the candidate extrema of the torques (fbr_candidate_extrema) instead of the torques -- the same route, the same kernels' arithmetic
static int run_id(fbr_model *m, const fbr_states *st, const double *x, int nx, const double *vel_sign, int mode,
                  double *tau_out, int32_t out_mem, const ExtremaReq *ext = nullptr)
{
    {
        std::vector<double> xr;
        int nxr = 0, rc = FBR_OK;
        if (fbr_model *r = merged_for_torques(m, st, x, nx, mode, xr, &nxr, &rc)) return run_id(r, st, xr.data(), nxr, vel_sign, mode, tau_out, out_mem, ext);
        if (rc) return rc;
    }
    DevStates d;
    int rc = stage_states(m, st, &d);
    if (rc) return rc;
    const FbrHostModel &hm = m->hm;
    if (!x || (!tau_out && !ext)) {
        set_err("null x / tau_out");
        return FBR_E_INVALID;
    }
    const int need = (mode == 0) ? (hm.fric ? hm.friction_start() + (hm.cols - hm.cpl * hm.L) : 10 * hm.L) : hm.cols;
    if (mode == 0 && nx < std::max(need, 10 * hm.L)) {
        set_err("x_std too short for this model layout");
        return FBR_E_INVALID;
    }
    const long S = d.S;
    if (S == 0) return FBR_OK;
    if ((rc = m->st_x.ensure((size_t)std::max(nx, 1) * sizeof(double)))) return rc;
    HIPCHK(hipMemcpyAsync(m->st_x.p, x, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, m->stream));
    const double *dvs = nullptr;
    if (mode == 0 && hm.fric && hm.stribeck > 0) {
        if (!vel_sign) {
            set_err("Stribeck model needs vel_sign");
            return FBR_E_INVALID;
        }
        if ((rc = stage_one(m, m->st_aux, vel_sign, (size_t)S * hm.n, st->mem, &dvs))) return rc;
    }
    DevKinExt ex;
    if (ext && (rc = extrema_tiles(m, S, ext->ncand, &ex))) return rc;
    double *dst = tau_out;
    if (ext ? !kinid_fits(m) : out_mem == FBR_HOST) {  // (extrema on the two-kernel route: the torques in a device temporary)
        if ((rc = m->out_tmp.ensure((size_t)S * hm.rows * sizeof(double)))) return rc;
        dst = m->out_tmp.as<double>();
    }
    if (kinid_fits(m)) {
        if ((rc = launch_kinid(m, d, S, dvs, m->st_x.as<double>(), mode, ext ? nullptr : dst, 0, nullptr, ext ? &ex : nullptr))) return rc;
        return ext ? finish_extrema(m, ex, *ext, out_mem) : finish_output(m, dst, tau_out, (size_t)S * hm.rows, out_mem);
    }
    if ((rc = launch_id_two_kernel(m, d, S, dvs, m->st_x.as<double>(), mode, dst))) return rc;
    if (ext) {
        {
            ProfScope ps(m, FBR_PROF_ID);
            hipLaunchKernelGGL(fbr_extrema_tiles_kernel, dim3((unsigned)std::min<long>(ex.nblk, (long)m->num_cus * 8)), dim3(256), 0, m->stream, ex, hm.n,
                               hm.fb, hm.rows, d.q, d.dq, (const double *)dst);
            HIPCHK(hipGetLastError());
        }
        return finish_extrema(m, ex, *ext, out_mem);
    }
    return finish_output(m, dst, tau_out, (size_t)S * hm.rows, out_mem);
}

extern "C" int fbr_inverse_dynamics_batch(fbr_model *m, const fbr_states *st, const double *x_std, int32_t num_x,
                                          const double *vel_sign, double *tau_out, int32_t out_mem)
{
    return run_id(m, st, x_std, num_x, vel_sign, 0, tau_out, out_mem);
}

extern "C" int fbr_candidate_extrema(fbr_model *m, const fbr_states *st, int32_t ncand, const double *x_std, int32_t num_x, const double *vel_sign,
                                     double *val_out, int64_t *idx_out, int32_t out_mem)
{
    if (!m || !st || !val_out || !idx_out) {
        set_err("null model / states / val_out / idx_out");
        return FBR_E_INVALID;
    }
    if (ncand < 1) {
        set_err("ncand must be at least 1");
        return FBR_E_INVALID;
    }
    if (st->num_samples <= 0 || st->num_samples % ncand != 0) {
        set_err("num_samples must be a positive multiple of ncand (equal candidates of consecutive samples)");
        return FBR_E_INVALID;
    }
    const ExtremaReq rq{ncand, val_out, idx_out};
    return run_id(m, st, x_std, num_x, vel_sign, 0, nullptr, out_mem, &rq);
}

// ---- torque rows of chosen samples under the finite-difference sweep (fbr.h; fbr_kintau_kernel, csrc/fbr_kinid.h) ------------------------
static int run_torque_sweep(fbr_model *m, const fbr_states *st, long ncand, long nrows, const int64_t *sample, const int32_t *joint, const double *x, int nx,
                            const double *vel_sign, double eps, double *out, int32_t out_mem)
{
    {
        std::vector<double> xr;
        int nxr = 0, rc = FBR_OK;
        if (fbr_model *r = merged_for_torques(m, st, x, nx, 0, xr, &nxr, &rc))
            return run_torque_sweep(r, st, ncand, nrows, sample, joint, xr.data(), nxr, vel_sign, eps, out, out_mem);
        if (rc) return rc;
    }
    DevStates d;
    int rc = stage_states(m, st, &d);
    if (rc) return rc;
    const FbrHostModel &hm = m->hm;
    const int n = hm.n, nper = 1 + 3 * n;
    const int need = hm.fric ? hm.friction_start() + (hm.cols - hm.cpl * hm.L) : 10 * hm.L;
    if (n < 1 || nx < std::max(need, 10 * hm.L)) {
        set_err("fbr_torque_row_sweep: a model without joints, or x_std too short for this model layout");
        return FBR_E_INVALID;
    }
    const long S = d.S, T = S / ncand, items = ncand * nrows;
    if ((rc = m->st_x.ensure((size_t)nx * sizeof(double)))) return rc;
    HIPCHK(hipMemcpyAsync(m->st_x.p, x, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, m->stream));
    const double *dx = m->st_x.as<double>(), *dvs = nullptr, *dsmp = nullptr;
    if (hm.fric && hm.stribeck > 0) {
        if (!vel_sign) {
            set_err("Stribeck model needs vel_sign");
            return FBR_E_INVALID;
        }
        if ((rc = stage_one(m, m->st_aux, vel_sign, (size_t)S * n, st->mem, &dvs))) return rc;
    }
    if ((rc = stage_one(m, m->st_aux2, (const double *)sample, (size_t)items, st->mem, &dsmp))) return rc;  // (8 bytes an entry, like a double)
    const int *djnt = joint;
    if (joint && st->mem == FBR_HOST) {
        if ((rc = m->st_bpos.ensure((size_t)items * sizeof(int32_t)))) return rc;
        HIPCHK(hipMemcpyAsync(m->st_bpos.p, joint, (size_t)items * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
        djnt = m->st_bpos.as<int>();
    }
    double *dout = out;
    if (out_mem == FBR_HOST) {
        if ((rc = m->g_tmp.ensure((size_t)items * nper * sizeof(double)))) return rc;
        dout = m->g_tmp.as<double>();
    }
    if ((rc = m->capg_flag.ensure(sizeof(int)))) return rc;
    int flag = 0;
    HIPCHK(hipMemsetAsync(m->capg_flag.p, 0, sizeof(int), m->stream));
    const DevKinTau tr{T, nrows, (const long *)dsmp, djnt, m->capg_flag.as<int>()};
    if (kinid_fits(m)) {
        // one lane per evaluation, nothing staged: no LDS, so the 105-DOF limit of the staged states does not apply, but kinid_fits is
        // the one rule for "the fused lane kernels serve this model"
        const DevKinId kp = kinid_params(m);
        const long nblk = (items * nper + 63) / 64;
        const int blocks = (int)std::min<long>(nblk, (long)m->num_cus * 8);
        if ((rc = m->kinid_scratch.ensure((size_t)blocks * std::max(kp.nslots, 1) * FBR_LINK_REC * 64 * sizeof(double)))) return rc;
        ProfScope ps(m, FBR_PROF_ID);
        fbr_by_depth<4, 8, 12, FBR_KINID_MAXD>(kp.maxlvl, [&](auto D) {
            hipLaunchKernelGGL(fbr_kintau_kernel<D>, dim3(blocks), dim3(64), 0, m->stream, m->dm, kp, tr, items, nper, eps, d.q, d.dq, d.ddq, d.bv, d.ba, d.rpy,
                               d.sign, dvs, dx, dout, m->kinid_scratch.as<double>());
        });
        HIPCHK(hipGetLastError());
    } else {
        // chunks of items whose expanded records stay within the usual chunk
        const long ch = std::max(1L, chunk_size(m, items * nper) / nper);
        const size_t cnt[7] = {(size_t)n, (size_t)n, (size_t)n, 6, 6, 3, (size_t)n};
        for (long i0 = 0; i0 < items; i0 += ch) {
            const long ci = std::min(ch, items - i0), ce = ci * nper;
            for (int i = 0; i < 7; i++)
                if ((rc = m->fd[i].ensure((size_t)ce * cnt[i] * sizeof(double)))) return rc;
            if ((rc = m->fd_part.ensure((size_t)ce * n * sizeof(double)))) return rc;           // vel_sign of the evaluations
            if ((rc = m->out_tmp.ensure((size_t)ce * hm.rows * sizeof(double)))) return rc;  // their torques
            DevStates de;
            de.S = ce;
            de.q = m->fd[0].as<double>();
            de.dq = m->fd[1].as<double>();
            de.ddq = m->fd[2].as<double>();
            if (d.bv) {
                de.bv = m->fd[3].as<double>();
                de.ba = m->fd[4].as<double>();
                de.rpy = m->fd[5].as<double>();
            }
            if (d.sign) de.sign = m->fd[6].as<double>();
            const unsigned grid = (unsigned)std::min<long>((ce + 255) / 256, 4096);
            hipLaunchKernelGGL(fbr_tau_expand_kernel, dim3(grid), dim3(256), 0, m->stream, tr, i0, ci, n, eps, d.q, d.dq, d.ddq, d.bv, d.ba, d.rpy, d.sign, dvs,
                               m->fd[0].as<double>(), m->fd[1].as<double>(), m->fd[2].as<double>(), m->fd[3].as<double>(), m->fd[4].as<double>(),
                               m->fd[5].as<double>(), m->fd[6].as<double>(), m->fd_part.as<double>());
            HIPCHK(hipGetLastError());
            if ((rc = launch_id_two_kernel(m, de, ce, dvs ? m->fd_part.as<double>() : nullptr, dx, 0, m->out_tmp.as<double>()))) return rc;
            hipLaunchKernelGGL(fbr_tau_gather_kernel, dim3(grid), dim3(256), 0, m->stream, tr, i0, ci, n, hm.fb, hm.rows, m->out_tmp.as<double>(), dout);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipMemcpyAsync(&flag, m->capg_flag.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    if ((rc = finish_output(m, dout, out, (size_t)items * nper, out_mem))) return rc;
    if (flag) {
        set_err("fbr_torque_row_sweep: a sample index lies outside 0 .. T - 1 or a joint index outside 0 .. n - 1");
        return FBR_E_INVALID;
    }
    return FBR_OK;
}

extern "C" int fbr_torque_row_sweep(fbr_model *m, const fbr_states *st, int32_t ncand, int64_t nrows, const int64_t *sample, const int32_t *joint,
                                    const double *x_std, int32_t num_x, const double *vel_sign, double eps, double *out, int32_t out_mem)
{
    if (!m || !st || !sample || !x_std || !out) {
        set_err("null model / states / sample / x_std / out");
        return FBR_E_INVALID;
    }
    if (out_mem != FBR_HOST && out_mem != FBR_DEVICE) {
        set_err("bad memory space of out");
        return FBR_E_INVALID;
    }
    if (ncand < 1 || nrows < 1) {
        set_err("ncand and nrows must be at least 1");
        return FBR_E_INVALID;
    }
    if (st->num_samples <= 0 || st->num_samples % ncand != 0) {
        set_err("num_samples must be a positive multiple of ncand (equal candidates of consecutive samples)");
        return FBR_E_INVALID;
    }
    if (!joint && nrows != m->hm.n) {
        set_err("joint == NULL needs nrows == number of joints");
        return FBR_E_INVALID;
    }
    if (!std::isfinite(eps) || eps == 0.0) {
        set_err("eps must be finite and not zero");
        return FBR_E_INVALID;
    }
    return run_torque_sweep(m, st, ncand, nrows, sample, joint, x_std, num_x, vel_sign, eps, out, out_mem);
}

// ---- base motion of a suspended robot (fbr.h; fbr_kinsusp_kernel + fbr_susp_scan_kernel, csrc/fbr_kinid.h) -------------------------------
// the argument checks both entry points share, then q / dq / ddq and the inertial parameters on the device and kernel 1: the records in
// m->susp_rec (or rec_dst, device memory, when given)
static int suspended_records(fbr_model *m, const fbr_states *st, const double *x_std, int32_t num_x, int32_t att_link, const char *who, double *rec_dst)
{
    if (st->num_samples < 0 || (st->mem != FBR_HOST && st->mem != FBR_DEVICE) || !st->q || !st->dq || !st->ddq) {
        set_err(std::string(who) + ": bad fbr_states header, or q / dq / ddq is NULL");
        return FBR_E_INVALID;
    }
    const FbrHostModel &hm = m->hm;
    if (!hm.floating) {
        set_err(std::string(who) + ": the model has no floating base");
        return FBR_E_INVALID;
    }
    if (att_link < 0 || att_link >= hm.L) {
        set_err(std::string(who) + ": att_link out of range");
        return FBR_E_INVALID;
    }
    if (num_x < 10 * hm.L) {
        set_err(std::string(who) + ": x_std too short (10 inertial parameters per link)");
        return FBR_E_INVALID;
    }
    if (!kinid_fits(m)) {
        set_err(std::string(who) + ": needs the one-lane-per-sample kernels -- option fused_id = 0, or joint paths of more than " +
                std::to_string(FBR_KINID_MAXD) + " joints; there is no two-kernel form");
        return FBR_E_UNSUPPORTED;
    }
    if (int rc = enter_blocking(m)) return rc;
    int rc;
    if (m->susp_att != att_link) {
        std::vector<char> keep(hm.L, 0);
        for (int a = att_link; a >= 0; a = hm.parent[a]) keep[a] = 1;
        try {
            fbr_kinid_build(hm, m->susp_prog, &keep);
        } catch (const std::exception &e) {
            set_err(e.what());
            return FBR_E_INVALID;
        }
        HIPCHK(hipStreamSynchronize(m->stream));
        m->susp_att = -1;
        if ((rc = m->susp_tab.ensure(m->susp_prog.steps.size() * sizeof(int)))) return rc;
        HIPCHK(hipMemcpy(m->susp_tab.p, m->susp_prog.steps.data(), m->susp_prog.steps.size() * sizeof(int), hipMemcpyHostToDevice));
        m->susp_att = att_link;
    }
    const long S = st->num_samples;
    const double *dq = nullptr, *ddq = nullptr, *dddq = nullptr;
    if ((rc = stage_one(m, m->st_q, st->q, (size_t)S * hm.n, st->mem, &dq))) return rc;
    if ((rc = stage_one(m, m->st_dq, st->dq, (size_t)S * hm.n, st->mem, &ddq))) return rc;
    if ((rc = stage_one(m, m->st_ddq, st->ddq, (size_t)S * hm.n, st->mem, &dddq))) return rc;
    if ((rc = m->st_x.ensure((size_t)10 * hm.L * sizeof(double)))) return rc;
    HIPCHK(hipMemcpyAsync(m->st_x.p, x_std, (size_t)10 * hm.L * sizeof(double), hipMemcpyHostToDevice, m->stream));
    if (!rec_dst) {
        if ((rc = m->susp_rec.ensure((size_t)S * FBR_SUSP_REC * sizeof(double)))) return rc;
        rec_dst = m->susp_rec.as<double>();
    }
    const DevKinId kp = kinid_params(m);
    const DevKinSusp su{att_link, m->susp_prog.nsteps, m->susp_prog.maxlvl, m->susp_tab.as<int>()};
    const long nblk = (S + 63) / 64;
    const int blocks = (int)std::min<long>(nblk, (long)m->num_cus * 8);
    if ((rc = m->kinid_scratch.ensure((size_t)blocks * std::max(std::max(kp.nslots, m->susp_prog.nslots), 1) * FBR_LINK_REC * 64 * sizeof(double)))) return rc;
    ProfScope ps(m, FBR_PROF_KIN);
    fbr_by_depth<4, 8, 12, FBR_KINID_MAXD>(kp.maxlvl, [&](auto D) {
        hipLaunchKernelGGL(fbr_kinsusp_kernel<D>, dim3(blocks), dim3(64), 0, m->stream, m->dm, kp, su, S, dq, ddq, dddq, (const double *)m->st_x.as<double>(),
                           rec_dst, m->kinid_scratch.as<double>());
    });
    HIPCHK(hipGetLastError());
    return FBR_OK;
}

extern "C" int fbr_suspended_records(fbr_model *m, const fbr_states *st, const double *x_std, int32_t num_x, int32_t att_link, double *rec_out,
                                     int32_t out_mem)
{
    if (!m || !st || !x_std || !rec_out || (out_mem != FBR_HOST && out_mem != FBR_DEVICE)) {
        set_err("fbr_suspended_records: null model / states / x_std / rec_out, or a bad memory space");
        return FBR_E_INVALID;
    }
    if (st->num_samples <= 0) {
        set_err("fbr_suspended_records: num_samples must be positive");
        return FBR_E_INVALID;
    }
    if (int rc = suspended_records(m, st, x_std, num_x, att_link, "fbr_suspended_records", out_mem == FBR_DEVICE ? rec_out : nullptr)) return rc;
    return finish_output(m, m->susp_rec.as<double>(), rec_out, (size_t)st->num_samples * FBR_SUSP_REC, out_mem);
}

extern "C" int fbr_suspended_base_motion(fbr_model *m, const fbr_states *st, int32_t ncand, const double *x_std, int32_t num_x, int32_t att_link,
                                         double dt, double damping, double *base_rpy, double *base_pos, double *base_vel, double *base_acc,
                                         double *att_state, int64_t *info, int32_t out_mem)
{
    if (!m || !st || !x_std || !base_rpy || !base_pos || !base_vel || !base_acc || (out_mem != FBR_HOST && out_mem != FBR_DEVICE)) {
        set_err("fbr_suspended_base_motion: null model / states / x_std / output, or a bad memory space");
        return FBR_E_INVALID;
    }
    if (!std::isfinite(dt) || dt <= 0.0 || !std::isfinite(damping) || damping < 0.0) {
        set_err("fbr_suspended_base_motion: dt must be finite and positive, damping finite and not negative");
        return FBR_E_INVALID;
    }
    if (ncand < 1) {
        set_err("fbr_suspended_base_motion: ncand must be at least 1");
        return FBR_E_INVALID;
    }
    if (st->num_samples <= 0 || st->num_samples % ncand != 0) {
        set_err("fbr_suspended_base_motion: num_samples must be a positive multiple of ncand (equal candidates of consecutive samples)");
        return FBR_E_INVALID;
    }
    if (int rc = suspended_records(m, st, x_std, num_x, att_link, "fbr_suspended_base_motion", nullptr)) return rc;
    const long S = st->num_samples, C = ncand, T = S / C;
    int rc;
    double *drpy = base_rpy, *dpos = base_pos, *dvel = base_vel, *dacc = base_acc, *datt = att_state;
    long *dinfo = (long *)info;
    if (out_mem == FBR_HOST) {
        // rpy 3 | pos 3 | vel 6 | acc 6 | att 6 per sample, then info
        if ((rc = m->susp_out.ensure((size_t)S * 24 * sizeof(double) + (size_t)C * 2 * sizeof(long)))) return rc;
        drpy = m->susp_out.as<double>();
        dpos = drpy + S * 3;
        dvel = dpos + S * 3;
        dacc = dvel + S * 6;
        datt = att_state ? dacc + S * 6 : nullptr;
        dinfo = info ? (long *)(dacc + S * 12) : nullptr;
    }
    const double *g = m->hm.gravity;
    {
        ProfScope ps(m, FBR_PROF_ID);
        hipLaunchKernelGGL(fbr_susp_scan_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, m->stream, C, T, g[0], g[1], g[2], dt, damping,
                           (const double *)m->susp_rec.as<double>(), drpy, dpos, dvel, datt, dinfo);
        HIPCHK(hipGetLastError());
    }
    {
        ProfScope ps(m, FBR_PROF_REDUCE);
        hipLaunchKernelGGL(fbr_susp_acc_kernel, dim3((unsigned)std::min<long>((S * 6 + 255) / 256, 4096)), dim3(256), 0, m->stream, C, T, dt,
                           (const double *)dvel, dacc);
        HIPCHK(hipGetLastError());
    }
    if (out_mem == FBR_HOST) {
        HIPCHK(hipMemcpyAsync(base_rpy, drpy, (size_t)S * 3 * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(base_pos, dpos, (size_t)S * 3 * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(base_vel, dvel, (size_t)S * 6 * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(base_acc, dacc, (size_t)S * 6 * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        if (att_state) HIPCHK(hipMemcpyAsync(att_state, datt, (size_t)S * 6 * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        if (info) HIPCHK(hipMemcpyAsync(info, dinfo, (size_t)C * 2 * sizeof(long), hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    prof_collect(m);
    return FBR_OK;
}

extern "C" int fbr_predict(fbr_model *m, const fbr_states *st, const double *x, double *tau_out, int32_t out_mem)
{
    if (!m) {
        set_err("null model");
        return FBR_E_INVALID;
    }
    return run_id(m, st, x, m->hm.cols, nullptr, 1, tau_out, out_mem);
}

extern "C" int fbr_contact_torques(fbr_model *m, const fbr_states *st, int32_t link, const double *frame_R,
                                   const double *frame_p, const double *wrench, double *out, int32_t out_mem)
{
    (void)frame_R;
    if (!m || !st) {
        set_err("null argument");
        return FBR_E_INVALID;
    }
    const FbrHostModel &hm = m->hm;
    if (link < 0 || link >= hm.L || !frame_p || !wrench || !out) {
        set_err("bad contact frame / null pointer");
        return FBR_E_INVALID;
    }
    fbr_states s2 = *st;
    // only q and rpy matter for the Jacobian: feed q as velocity placeholders (never read into the result)
    s2.dq = st->q;
    s2.ddq = st->q;
    if (hm.floating) {
        s2.base_vel = nullptr;
        s2.base_acc = nullptr;
    }
    s2.sign = nullptr;
    DevStates d;
    int rc = stage_states(m, &s2, &d, false);
    if (rc) return rc;
    const long S = d.S;
    if (S == 0) return FBR_OK;
    if (hm.floating) {
        // zero twist / acceleration buffers
        if ((rc = m->st_bv.ensure((size_t)S * 6 * sizeof(double)))) return rc;
        HIPCHK(hipMemsetAsync(m->st_bv.p, 0, (size_t)S * 6 * sizeof(double), m->stream));
        d.bv = d.ba = m->st_bv.as<double>();
    }
    const double *dw = nullptr;
    if ((rc = stage_one(m, m->st_aux, wrench, (size_t)S * 6, st->mem, &dw))) return rc;
    double *dst = out;
    if (out_mem == FBR_HOST) {
        if ((rc = m->out_tmp.ensure((size_t)S * hm.rows * sizeof(double)))) return rc;
        dst = m->out_tmp.as<double>();
    }
    if (kinid_fits(m)) {  // the same fused kernel: only the frame's link carries a wrench (fbr_kinid.h, mode 2)
        if ((rc = launch_kinid(m, d, S, nullptr, dw, 2, dst, link, frame_p))) return rc;
        return finish_output(m, dst, out, (size_t)S * hm.rows, out_mem);
    }
    const long ch = chunk_size(m, S);
    for (long s0 = 0; s0 < S; s0 += ch) {
        const long cs = std::min(ch, S - s0);
        if ((rc = run_kin(m, d, s0, cs))) return rc;
        hipLaunchKernelGGL(fbr_contact_kernel, dim3((unsigned)((cs + 255) / 256)), dim3(256), 0, m->stream, m->dm, cs,
                           m->rec.as<double>(), link, frame_p[0], frame_p[1], frame_p[2], dw + s0 * 6,
                           dst + (size_t)s0 * hm.rows);
        HIPCHK(hipGetLastError());
    }
    return finish_output(m, dst, out, (size_t)S * hm.rows, out_mem);
}
// ngroups > 1: the samples form ngroups consecutive groups of equal size, one Gram per group (G_out [ngroups][Pa][Pa])
// Which regressor rows carry a non-zero weight for at least one sample (device scan of w; all rows when there are no weights).
int active_rows(fbr_model *m, const double *dw, long S, std::vector<char> *act)
{
    const int rows = m->hm.rows;
    act->assign(rows, 1);
    if (!dw || S <= 0) return FBR_OK;
    int rc;
    if ((rc = m->row_flags.ensure((size_t)rows * sizeof(int)))) return rc;
    HIPCHK(hipMemsetAsync(m->row_flags.p, 0, (size_t)rows * sizeof(int), m->stream));
    hipLaunchKernelGGL(fbr_row_active_kernel, dim3(1024), dim3(256), 0, m->stream, dw, S, rows, m->row_flags.as<int>());
    HIPCHK(hipGetLastError());
    std::vector<int> h(rows);
    HIPCHK(hipMemcpyAsync(h.data(), m->row_flags.p, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    for (int r = 0; r < rows; r++) (*act)[r] = h[r] != 0;
    return FBR_OK;
}
// Block until the submission with this ticket (and every earlier one) is complete; ticket < 0 or beyond the last one: everything.
int wait_ticket(fbr_model *m, int64_t ticket)
{
    const int64_t last = m->next_ticket - 1;
    if (ticket > last) ticket = last;
    if (ticket <= m->waited_ticket) return FBR_OK;
    // the completion event is what carries the submission (recorded on the stream it ran on, whatever m->stream is by now)
    HIPCHK(hipEventSynchronize(m->ev_done[ticket & 1]));
    if (ticket == last) {
        HIPCHK(hipStreamSynchronize(m->stream));
        HIPCHK(hipStreamSynchronize(m->side));
        if (m->copy) HIPCHK(hipStreamSynchronize(m->copy));
        prof_collect(m);
    }
    const int64_t first = m->waited_ticket + 1;
    m->waited_ticket = ticket;
    for (int64_t t = std::max(first, ticket - 1); t <= ticket; t++)
        if (m->ticket_via_red[t & 1]) {  // the pass ran on a reduced model: its bookkeeping, profile and error word
            fbr_model *r = m->rdm[m->ticket_via_red[t & 1] - 1].get();
            m->ticket_via_red[t & 1] = 0;
            if (int rc = wait_ticket(r, m->red_ticket[t & 1])) return rc;
        }
    for (int64_t t = std::max(first, ticket - 1); t <= ticket; t++)  // (at most two submissions were in flight)
        if (m->ticket_kind[t & 1] == 1 && m->tsqr_err_host && m->tsqr_err_host[t & 1]) {
            char hx[16];
            snprintf(hx, sizeof hx, "%08x", m->tsqr_err_host[t & 1]);
            m->tsqr_err_host[t & 1] = 0;
            set_err("TSQR pipeline flag wait timed out (internal error, code " + std::string(hx) + ") in submission " + std::to_string(t));
            return FBR_E_HIP;
        }
    return FBR_OK;
}
extern "C" int fbr_wait(fbr_model *m, int64_t ticket)
{
    int rc = enter(m);
    if (rc) return rc;
    return wait_ticket(m, ticket < 0 ? m->next_ticket - 1 : ticket);
}

extern "C" int fbr_fd_scores(fbr_model *m, const fbr_states *st, const double *W, double eps, double *out, int32_t out_mem)
{
    DevStates d;
    int rc = stage_states(m, st, &d);
    if (rc) return rc;
    if (!W || !out) {
        set_err("W / out is NULL");
        return FBR_E_INVALID;
    }
    const FbrHostModel &hm = m->hm;
    const long S = d.S;
    const int n = hm.n, nper = 1 + 3 * n;
    const double *dW = nullptr;
    if ((rc = stage_one(m, m->st_aux, W, (size_t)S * hm.rows * hm.cols, st->mem, &dW))) return rc;
    double *dout = out;
    if (out_mem == FBR_HOST) {
        if ((rc = m->g_tmp.ensure((size_t)S * nper * sizeof(double)))) return rc;
        dout = m->g_tmp.as<double>();
    }
    if (S > 0 && m->opt.fused_id != 0 && m->kinid.nsteps > 0 && !hm.masked) {
        // one lane per evaluation, nothing staged (fbr_kinfd_kernel, fbr_kinid.h)
        const DevKinId kp = kinid_params(m);
        const long nblk = (S * nper + 63) / 64;
        const int blocks = (int)std::min<long>(nblk, (long)m->num_cus * 8);
        if ((rc = m->kinid_scratch.ensure((size_t)blocks * std::max(kp.nslots, 1) * FBR_LINK_REC * 64 * sizeof(double)))) return rc;
        {
            ProfScope ps(m, FBR_PROF_REGRESSOR);
            fbr_by_depth<4, 8, 12, FBR_KINID_MAXD>(kp.maxlvl, [&](auto D) {
                hipLaunchKernelGGL(fbr_kinfd_kernel<D>, dim3(blocks), dim3(64), 0, m->stream, m->dm, kp, S, nper, eps, d.q, d.dq, d.ddq, d.bv, d.ba,
                                   d.rpy, d.sign, dW, dout, m->kinid_scratch.as<double>());
            });
        }
        HIPCHK(hipGetLastError());
    } else if (S > 0) {
        // columns that a perturbation of joint d can change: the inertial columns of the links below d and d's own friction columns
        if (m->fd_tab_entries < 0) {
            std::vector<int> tab(n + 1, 0), ent;
            for (int dj = 0; dj < n; dj++) {
                tab[dj] = (int)ent.size();
                for (int c = 0; c < hm.cols; c++) {
                    const FbrCol &cd = hm.coldesc[c];
                    const bool on = cd.kind == 0 ? std::find(hm.path[cd.link].begin(), hm.path[cd.link].end(), dj) != hm.path[cd.link].end() : cd.joint == dj;
                    if (on) ent.push_back(c);
                }
            }
            tab[n] = (int)ent.size();
            tab.insert(tab.end(), ent.begin(), ent.end());
            if ((rc = m->fd_tab.ensure(tab.size() * sizeof(int)))) return rc;
            HIPCHK(hipMemcpyAsync(m->fd_tab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipStreamSynchronize(m->stream));  // tab is a local
            m->fd_tab_entries = (int)ent.size();
        }
        const int *jbeg = m->fd_tab.as<int>(), *jcols = jbeg + n + 1;
        // chunks of original samples such that the expanded kinematic records stay within the usual chunk
        long ch = std::max(1L, chunk_size(m, S * nper) / nper);
        if ((rc = m->fd_part.ensure((size_t)std::min(ch, S) * std::max(n, 1) * sizeof(double)))) return rc;
        const size_t lds = ((size_t)hm.rec_size() + 4 + hm.cols) * sizeof(double);
        HIPCHK(hipFuncSetAttribute((const void *)fbr_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const size_t cnt[7] = {(size_t)n, (size_t)n, (size_t)n, 6, 6, 3, (size_t)n};
        for (long s0 = 0; s0 < S; s0 += ch) {
            const long cs = std::min(ch, S - s0), ce = cs * nper;
            for (int i = 0; i < 7; i++)
                if ((rc = m->fd[i].ensure((size_t)ce * cnt[i] * sizeof(double)))) return rc;
            hipLaunchKernelGGL(fbr_fd_expand_kernel, dim3((unsigned)std::min<long>((ce + 255) / 256, 4096)), dim3(256), 0, m->stream, cs, n,
                               d.bv ? 1 : 0, d.sign ? 1 : 0, eps, d.q + s0 * n, d.dq + s0 * n, d.ddq + s0 * n, d.bv ? d.bv + s0 * 6 : nullptr,
                               d.ba ? d.ba + s0 * 6 : nullptr, d.rpy ? d.rpy + s0 * 3 : nullptr, d.sign ? d.sign + s0 * n : nullptr,
                               m->fd[0].as<double>(), m->fd[1].as<double>(), m->fd[2].as<double>(), m->fd[3].as<double>(),
                               m->fd[4].as<double>(), m->fd[5].as<double>(), m->fd[6].as<double>());
            HIPCHK(hipGetLastError());
            DevStates de;
            de.S = ce;
            de.q = m->fd[0].as<double>();
            de.dq = m->fd[1].as<double>();
            de.ddq = m->fd[2].as<double>();
            if (d.bv) {
                de.bv = m->fd[3].as<double>();
                de.ba = m->fd[4].as<double>();
                de.rpy = m->fd[5].as<double>();
            }
            if (d.sign) de.sign = m->fd[6].as<double>();
            if ((rc = run_kin(m, de, 0, ce))) return rc;
            {
                ProfScope ps(m, FBR_PROF_REGRESSOR);
                for (int phase = 0; phase < (n > 0 ? 2 : 1); phase++)
                    hipLaunchKernelGGL(fbr_score_kernel, dim3((unsigned)std::min<long>(phase ? cs * (nper - 1) : cs, (long)m->num_cus * 8)), dim3(256), lds,
                                       m->stream, m->dm, cs, nper, phase, m->rec.as<double>(), de.dq, de.sign, dW + (size_t)s0 * hm.rows * hm.cols,
                                       dout + (size_t)s0 * nper, m->fd_part.as<double>(), jbeg, jcols);
            }
            HIPCHK(hipGetLastError());
        }
    }
    return finish_output(m, dout, out, (size_t)S * nper, out_mem);
}
// ------------------------------------------------------------------------------------------------
// Fourier-series states of candidate trajectories, generated on the device (fbr.h)
// ------------------------------------------------------------------------------------------------
extern "C" int fbr_fourier_states(fbr_model *m, int32_t ncand, int64_t T, int32_t nharm, double freq, const double *wf, const double *a, const double *b,
                                  const double *q_offset, const double *q_range, double *q, double *dq, double *ddq, int32_t out_mem)
{
    if (!m || ncand < 1 || T < 1 || nharm < 1 || !(freq > 0) || !wf || !a || !b || !q_offset || !q || !dq || !ddq ||
        (out_mem != FBR_HOST && out_mem != FBR_DEVICE)) {
        set_err("fbr_fourier_states: bad arguments");
        return FBR_E_INVALID;
    }
    if (int rc = enter_blocking(m)) return rc;
    const int n = m->hm.n;
    const size_t nc = (size_t)ncand * n, ncoef = nc * nharm, count = (size_t)ncand * (size_t)T * n;
    // coefficients: [wf (C) | a | b | q_offset | q_range] in one staging buffer (host arrays, a few KB)
    std::vector<double> h;
    h.insert(h.end(), wf, wf + ncand);
    h.insert(h.end(), a, a + ncoef);
    h.insert(h.end(), b, b + ncoef);
    h.insert(h.end(), q_offset, q_offset + nc);
    if (q_range) h.insert(h.end(), q_range, q_range + nc);
    int rc;
    if ((rc = m->st_x.ensure(h.size() * sizeof(double)))) return rc;
    HIPCHK(hipMemcpyAsync(m->st_x.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));  // (h is a local)
    const double *d = m->st_x.as<double>();
    const double *dwf = d, *da = d + ncand, *db = da + ncoef, *doff = db + ncoef, *drng = q_range ? doff + nc : nullptr;
    double *oq = q, *odq = dq, *oddq = ddq;
    if (out_mem == FBR_HOST) {
        if ((rc = m->out_tmp.ensure(3 * count * sizeof(double)))) return rc;
        oq = m->out_tmp.as<double>();
        odq = oq + count;
        oddq = odq + count;
    }
    hipLaunchKernelGGL(fbr_fourier_kernel, dim3((unsigned)std::min<size_t>((count + 255) / 256, (size_t)m->num_cus * 32)), dim3(256), 0, m->stream, (int)ncand, (long)T, n,
                       (int)nharm, freq, dwf, da, db, doff, drng, oq, odq, oddq);
    HIPCHK(hipGetLastError());
    if (out_mem == FBR_HOST) {
        HIPCHK(hipMemcpyAsync(q, oq, count * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(dq, odq, count * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(ddq, oddq, count * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    return FBR_OK;
}

// ------------------------------------------------------------------------------------------------
// D-optimality weight rows W = Y[:, cols] . C_g of the analytical trajectory gradient (fbr.h; kernel and tiling: fbr_weights.h)
// ------------------------------------------------------------------------------------------------
extern "C" int fbr_regressor_weights(fbr_model *m, const fbr_states *st, int32_t ngroups, const int32_t *cols, int32_t ncols, const double *C,
                                     double *W, int32_t mem)
{
    DevStates d;
    int rc = stage_states(m, st, &d);
    if (rc) return rc;
    const FbrHostModel &hm = m->hm;
    const int P = hm.cols;
    if (!cols) ncols = P;
    if (!W || !C || ngroups < 1 || ncols < 1 || ncols > P || (mem != FBR_HOST && mem != FBR_DEVICE)) {
        set_err("fbr_regressor_weights: W / C is NULL, ngroups < 1, ncols outside 1 .. cols or a bad memory space");
        return FBR_E_INVALID;
    }
    const long S = d.S;
    if (S % ngroups) {
        set_err("fbr_regressor_weights: num_samples must be a multiple of ngroups");
        return FBR_E_INVALID;
    }
    // device tables [cols (ncols) | columns not selected (P - ncols)]
    std::vector<int> tab;
    if (cols) {
        std::vector<char> seen(P, 0);
        for (int i = 0; i < ncols; i++) {
            if (cols[i] < 0 || cols[i] >= P || seen[cols[i]]) {
                set_err("fbr_regressor_weights: cols holds an index out of range or twice");
                return FBR_E_INVALID;
            }
            seen[cols[i]] = 1;
            tab.push_back(cols[i]);
        }
        for (int c = 0; c < P; c++)
            if (!seen[c]) tab.push_back(c);
    }
    const int mt = fbr_weights_mt(ncols);
    if (!mt) {
        set_err("fbr_regressor_weights: a 16-row tile of the selected columns exceeds the LDS (at most 1196 columns)");
        return FBR_E_UNSUPPORTED;
    }
    if (S == 0) return FBR_OK;
    DevWeights wp;
    wp.Rg = (S / ngroups) * hm.rows;
    wp.P = P;
    wp.ncols = ncols;
    wp.ldk = fbr_weights_ldk(ncols);
    wp.nunsel = cols ? P - ncols : 0;
    wp.cols = wp.unsel = nullptr;
    if (cols) {
        if ((rc = m->wt_tab.ensure(tab.size() * sizeof(int)))) return rc;
        HIPCHK(hipMemcpyAsync(m->wt_tab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));  // (tab is a local)
        wp.cols = m->wt_tab.as<int>();
        wp.unsel = wp.cols + ncols;
    }
    if ((rc = stage_one(m, m->st_aux, C, (size_t)ngroups * ncols * ncols, st->mem, &wp.C))) return rc;
    const size_t per = (size_t)hm.rows * P, lds = (size_t)16 * mt * wp.ldk * sizeof(double);
    long ch = chunk_size(m, S);
    if (mem == FBR_HOST) {  // as fbr_regressor_batch: the device copy of a chunk of the output stays within ~1 GiB
        ch = std::max(1L, std::min(ch, (long)((size_t)(1u << 30) / (per * sizeof(double)))));
        if ((rc = m->out_tmp.ensure((size_t)ch * per * sizeof(double)))) return rc;
    }
    void (*kern)(DevWeights, double *) = mt == 4 ? fbr_weights_kernel<4> : mt == 2 ? fbr_weights_kernel<2> : fbr_weights_kernel<1>;
    HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (long s0 = 0; s0 < S; s0 += ch) {
        const long cs = std::min(ch, S - s0);
        if ((rc = run_kin(m, d, s0, cs))) return rc;
        double *dst = (mem == FBR_HOST) ? m->out_tmp.as<double>() : W + (size_t)s0 * per;
        if ((rc = launch_regressor(m, d, s0, cs, dst, P, (long)hm.rows, 1L, nullptr, nullptr))) return rc;
        wp.R0 = s0 * hm.rows;
        wp.R1 = (s0 + cs) * hm.rows;
        const long tiles = fbr_weights_tiles(&wp, mt);
        {
            ProfScope ps(m, FBR_PROF_GRAM);
            hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(256), lds, m->stream, wp, dst);
        }
        HIPCHK(hipGetLastError());
        if (mem == FBR_HOST) {
            HIPCHK(hipMemcpyAsync(W + (size_t)s0 * per, dst, (size_t)cs * per * sizeof(double), hipMemcpyDeviceToHost, m->stream));
            HIPCHK(hipStreamSynchronize(m->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    prof_collect(m);
    return FBR_OK;
}

// ------------------------------------------------------------------------------------------------
// Chain of the sensitivities with the Jacobian of the Fourier series (fbr.h; kernels beside fbr_fourier_kernel, fbr_kernels.h)
// ------------------------------------------------------------------------------------------------
extern "C" int fbr_fourier_gradient(fbr_model *m, int32_t ncand, int64_t T, int32_t tstride, int32_t nharm, double freq, const double *wf,
                                    const double *a, const double *b, const double *q_range, const double *sens_q, const double *sens_dq,
                                    const double *sens_ddq, int32_t sens_mem, double *out, int32_t out_mem)
{
    if (!m || ncand < 1 || T < 1 || tstride < 1 || nharm < 1 || !(freq > 0) || !wf || !a || !b || !sens_q || !sens_dq || !sens_ddq || !out ||
        (sens_mem != FBR_HOST && sens_mem != FBR_DEVICE) || (out_mem != FBR_HOST && out_mem != FBR_DEVICE)) {
        set_err("fbr_fourier_gradient: bad arguments");
        return FBR_E_INVALID;
    }
    if (int rc = enter_blocking(m)) return rc;
    const int n = m->hm.n, K = 3 + 2 * nharm;
    const size_t nc = (size_t)ncand * n, ncoef = nc * nharm, count = (size_t)ncand * (size_t)T * n, nout = (size_t)ncand * (1 + 2 * n + 2 * (size_t)n * nharm);
    std::vector<double> h;  // [wf (C) | a | b | q_range]
    h.insert(h.end(), wf, wf + ncand);
    h.insert(h.end(), a, a + ncoef);
    h.insert(h.end(), b, b + ncoef);
    if (q_range) h.insert(h.end(), q_range, q_range + nc);
    int rc;
    if ((rc = m->st_x.ensure(h.size() * sizeof(double)))) return rc;
    HIPCHK(hipMemcpyAsync(m->st_x.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));  // (h is a local)
    const double *dc = m->st_x.as<double>();
    const double *dwf = dc, *da = dc + ncand, *db = da + ncoef, *drng = q_range ? db + ncoef : nullptr;
    const double *dsq, *dsdq, *dsddq;
    if ((rc = stage_one(m, m->st_q, sens_q, count, sens_mem, &dsq))) return rc;
    if ((rc = stage_one(m, m->st_dq, sens_dq, count, sens_mem, &dsdq))) return rc;
    if ((rc = stage_one(m, m->st_ddq, sens_ddq, count, sens_mem, &dsddq))) return rc;
    // samples per block: 64, halved until the five staged factors of a block fit 64 KiB of LDS
    int TB = 64;
    while (TB > 1 && (size_t)5 * TB * n * sizeof(double) > (size_t)64 * 1024) TB >>= 1;
    const size_t lds = (size_t)5 * TB * n * sizeof(double);
    if (lds > (size_t)160 * 1024) {
        set_err("fbr_fourier_gradient: more than 4096 joints");
        return FBR_E_UNSUPPORTED;
    }
    const long ntb = (long)((T + TB - 1) / TB), nblk = (long)ncand * ntb;
    if ((rc = m->fgrad_part.ensure((size_t)nblk * n * K * sizeof(double)))) return rc;
    double *dout = out;
    if (out_mem == FBR_HOST) {
        if ((rc = m->g_tmp.ensure(nout * sizeof(double)))) return rc;
        dout = m->g_tmp.as<double>();
    }
    {
        ProfScope ps(m, FBR_PROF_REDUCE);
        HIPCHK(hipFuncSetAttribute((const void *)fbr_fourier_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(fbr_fourier_grad_kernel, dim3((unsigned)std::min<long>(nblk, (long)m->num_cus * 16)), dim3(256), lds, m->stream, (int)ncand, (long)T,
                           (int)tstride, n, (int)nharm, TB, ntb, freq, dwf, da, db, drng, dsq, dsdq, dsddq, m->fgrad_part.as<double>());
        hipLaunchKernelGGL(fbr_fourier_grad_finish_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, m->stream, (int)ncand, n, (int)nharm, ntb,
                           m->fgrad_part.as<double>(), dout);
    }
    HIPCHK(hipGetLastError());
    return finish_output(m, dout, out, nout, out_mem);
}

// ------------------------------------------------------------------------------------------------
// Chain of position sensitivities at single times with the position Jacobian of the Fourier series (fbr.h; fbr_fourier_poschain_kernel)
// ------------------------------------------------------------------------------------------------
extern "C" int fbr_fourier_position_chain(fbr_model *m, int32_t ncand, int64_t nrows, int32_t nharm, double freq, const double *wf, const double *a,
                                          const double *b, const double *q_range, const int64_t *sample, const double *scale, const double *grad_q,
                                          int32_t mem, double *out, int32_t out_mem)
{
    if (!m || ncand < 1 || nrows < 1 || nharm < 1 || !(freq > 0) || !wf || !a || !b || !sample || !grad_q || !out ||
        (mem != FBR_HOST && mem != FBR_DEVICE) || (out_mem != FBR_HOST && out_mem != FBR_DEVICE)) {
        set_err("fbr_fourier_position_chain: bad arguments");
        return FBR_E_INVALID;
    }
    if (int rc = enter_blocking(m)) return rc;
    const int n = m->hm.n;
    const size_t nc = (size_t)ncand * n, ncoef = nc * nharm, rows = (size_t)ncand * (size_t)nrows, E = 1 + 2 * (size_t)n + 2 * (size_t)n * nharm,
                 nout = rows * E;
    std::vector<double> h;  // [wf (C) | a | b | q_range]
    h.insert(h.end(), wf, wf + ncand);
    h.insert(h.end(), a, a + ncoef);
    h.insert(h.end(), b, b + ncoef);
    if (q_range) h.insert(h.end(), q_range, q_range + nc);
    int rc;
    if ((rc = m->st_x.ensure(h.size() * sizeof(double)))) return rc;
    HIPCHK(hipMemcpyAsync(m->st_x.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));  // (h is a local)
    const double *dc = m->st_x.as<double>();
    const double *dwf = dc, *da = dc + ncand, *db = da + ncoef, *drng = q_range ? db + ncoef : nullptr;
    const double *dsmp, *dscale, *dg;
    if ((rc = stage_one(m, m->st_dq, (const double *)sample, rows, mem, &dsmp))) return rc;  // (8 bytes an entry, like a double)
    if ((rc = stage_one(m, m->st_aux, scale, rows, mem, &dscale))) return rc;
    if ((rc = stage_one(m, m->st_q, grad_q, rows * n, mem, &dg))) return rc;
    double *dout = out;
    if (out_mem == FBR_HOST) {
        if ((rc = m->g_tmp.ensure(nout * sizeof(double)))) return rc;
        dout = m->g_tmp.as<double>();
    }
    {
        ProfScope ps(m, FBR_PROF_REDUCE);
        hipLaunchKernelGGL(fbr_fourier_poschain_kernel, dim3((unsigned)std::min<size_t>((nout + 255) / 256, (size_t)m->num_cus * 32)), dim3(256), 0, m->stream,
                           (int)ncand, (long)nrows, n, (int)nharm, freq, dwf, da, db, drng, (const long *)dsmp, dscale, dg, dout);
    }
    HIPCHK(hipGetLastError());
    return finish_output(m, dout, out, nout, out_mem);
}

// ------------------------------------------------------------------------------------------------
// The same chain for rows that carry velocity and acceleration sensitivities as well (fbr.h; fbr_fourier_statechain_kernel)
// ------------------------------------------------------------------------------------------------
extern "C" int fbr_fourier_state_chain(fbr_model *m, int32_t ncand, int64_t nrows, int32_t nharm, double freq, const double *wf, const double *a,
                                       const double *b, const double *q_range, const int64_t *sample, const double *scale, const double *grad_q,
                                       const double *grad_dq, const double *grad_ddq, int32_t mem, double *out, int32_t out_mem)
{
    if (!m || ncand < 1 || nrows < 1 || nharm < 1 || !(freq > 0) || !wf || !a || !b || !sample || !out || (mem != FBR_HOST && mem != FBR_DEVICE) ||
        (out_mem != FBR_HOST && out_mem != FBR_DEVICE)) {
        set_err("fbr_fourier_state_chain: bad arguments");
        return FBR_E_INVALID;
    }
    if (int rc = enter_blocking(m)) return rc;
    const int n = m->hm.n;
    const size_t nc = (size_t)ncand * n, ncoef = nc * nharm, rows = (size_t)ncand * (size_t)nrows, E = 1 + 2 * (size_t)n + 2 * (size_t)n * nharm,
                 nout = rows * E;
    std::vector<double> h;  // [wf (C) | a | b | q_range]
    h.insert(h.end(), wf, wf + ncand);
    h.insert(h.end(), a, a + ncoef);
    h.insert(h.end(), b, b + ncoef);
    if (q_range) h.insert(h.end(), q_range, q_range + nc);
    int rc;
    if ((rc = m->st_x.ensure(h.size() * sizeof(double)))) return rc;
    HIPCHK(hipMemcpyAsync(m->st_x.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));  // (h is a local)
    const double *dc = m->st_x.as<double>();
    const double *dwf = dc, *da = dc + ncand, *db = da + ncoef, *drng = q_range ? db + ncoef : nullptr;
    const double *dsmp, *dscale, *dg, *dgd, *dgdd;
    if ((rc = stage_one(m, m->st_aux2, (const double *)sample, rows, mem, &dsmp))) return rc;  // (8 bytes an entry, like a double)
    if ((rc = stage_one(m, m->st_aux, scale, rows, mem, &dscale))) return rc;
    if ((rc = stage_one(m, m->st_q, grad_q, rows * n, mem, &dg))) return rc;
    if ((rc = stage_one(m, m->st_dq, grad_dq, rows * n, mem, &dgd))) return rc;
    if ((rc = stage_one(m, m->st_ddq, grad_ddq, rows * n, mem, &dgdd))) return rc;
    double *dout = out;
    if (out_mem == FBR_HOST) {
        if ((rc = m->g_tmp.ensure(nout * sizeof(double)))) return rc;
        dout = m->g_tmp.as<double>();
    }
    {
        ProfScope ps(m, FBR_PROF_REDUCE);
        hipLaunchKernelGGL(fbr_fourier_statechain_kernel, dim3((unsigned)std::min<size_t>((nout + 255) / 256, (size_t)m->num_cus * 32)), dim3(256), 0, m->stream,
                           (int)ncand, (long)nrows, n, (int)nharm, freq, dwf, da, db, drng, (const long *)dsmp, dscale, dg, dgd, dgdd, dout);
    }
    HIPCHK(hipGetLastError());
    return finish_output(m, dout, out, nout, out_mem);
}

// A submission that fails after work was enqueued has no ticket its caller could wait on: everything in flight is drained before the
// error is returned (the same for the Gram pass, gram_impl below), so that the inputs may be freed and later calls start from a quiet device.
int drain_after_failed_submit(fbr_model *m)
{
    if (!m) return FBR_OK;
    for (auto &r : m->rdm)
        if (r) drain_after_failed_submit(r.get());
    m->ticket_via_red[0] = m->ticket_via_red[1] = 0;
    (void)hipStreamSynchronize(m->stream);
    if (m->side) (void)hipStreamSynchronize(m->side);
    if (m->copy) (void)hipStreamSynchronize(m->copy);
    if (m->tsqr_pro_stream) (void)hipStreamSynchronize(m->tsqr_pro_stream);
    for (auto &s2 : m->tsqr_streams)
        if (s2) (void)hipStreamSynchronize(s2);
    m->waited_ticket = m->next_ticket - 1;
    m->ev_gram_rec[0] = m->ev_gram_rec[1] = m->ev_pack_rec[0] = m->ev_pack_rec[1] = false;
    m->tsqr_l0_rec = false;
    return FBR_OK;
}
