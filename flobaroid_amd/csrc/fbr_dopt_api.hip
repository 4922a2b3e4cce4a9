// fbr_dopt_api.hip -- fbr_dopt_terms: eigenvalues, D-optimality terms and weight matrices of candidate Grams; fbr_dopt_observability: their
// eigenvectors and the observability analysis built on them (kernel text: fbr_dopt.h).
#include "fbr_internal.h"
#include "fbr_dopt.h"

// the refusals every entry point of this file shares; `fn`: the name the message starts with
static int dopt_check(const char *fn, const fbr_model *m, const void *G, int32_t ngroups, int32_t Pa, const int32_t *cols, int32_t ncols, const void *out,
                      const char *out_name, int32_t mem)
{
    const std::string f(fn);
    if (ngroups < 1) {
        set_err(f + ": ngroups < 1");
        return FBR_E_INVALID;
    }
    if (!m || !G || !cols || !out || (mem != FBR_HOST && mem != FBR_DEVICE)) {
        set_err(f + ": m / G / cols / " + out_name + " is NULL or a bad memory space");
        return FBR_E_INVALID;
    }
    if (ncols < 1 || ncols > Pa) {
        set_err(f + ": ncols outside 1 .. Pa");
        return FBR_E_INVALID;
    }
    if (ncols > FBR_MAX_DOPT_COLUMNS) {
        set_err(f + ": " + std::to_string(ncols) + " columns, more than FBR_MAX_DOPT_COLUMNS = " + std::to_string(FBR_MAX_DOPT_COLUMNS));
        return FBR_E_INVALID;
    }
    std::vector<char> seen(Pa, 0);
    for (int i = 0; i < ncols; i++) {
        if (cols[i] < 0 || cols[i] >= Pa || seen[cols[i]]) {
            set_err(f + ": cols holds an index out of range or twice");
            return FBR_E_INVALID;
        }
        seen[cols[i]] = 1;
    }
    return FBR_OK;
}

extern "C" int fbr_dopt_terms(fbr_model *m, const double *G, int32_t ngroups, int32_t Pa, const int32_t *cols, int32_t ncols, const double *prior,
                              double reg, const double *scale, double *terms, int32_t *status, double *eig, double *Cmat, int32_t mem)
{
    if (int rc_check = dopt_check("fbr_dopt_terms", m, G, ngroups, Pa, cols, ncols, terms, "terms", mem)) return rc_check;
    if (!(reg >= 0.0) || !(reg <= DBL_MAX)) {
        set_err("fbr_dopt_terms: reg is negative or not finite");
        return FBR_E_INVALID;
    }
    if (int rc_enter = enter_blocking(m)) return rc_enter;
    int rc;
    const size_t n = (size_t)ncols, nn = n * n, gg = (size_t)Pa * Pa;
    // [scale | cols] of the call on the device
    const size_t sbytes = scale ? (size_t)ngroups * sizeof(double) : 0;
    std::vector<char> tab(sbytes + n * sizeof(int));
    if (scale) memcpy(tab.data(), scale, sbytes);
    memcpy(tab.data() + sbytes, cols, n * sizeof(int));
    if ((rc = m->dopt_tab.ensure(tab.size()))) return rc;
    HIPCHK(hipMemcpyAsync(m->dopt_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));  // (tab is a local)
    // candidates per launch: no grid dimension above 65535, the scratch within 256 MiB, the staged Grams of a host call within 1 GiB
    long ch = std::min<long>(65535, std::max<long>(1, (long)(((size_t)256 << 20) / (nn * sizeof(double)))));
    if (mem == FBR_HOST) ch = std::min<long>(ch, std::max<long>(1, (long)(((size_t)1 << 30) / (gg * sizeof(double)))));
    ch = std::min<long>(ch, ngroups);
    if ((rc = m->dopt_scratch.ensure((size_t)ch * nn * sizeof(double)))) return rc;
    DevDopt p;
    p.Pa = Pa, p.n = ncols, p.reg = reg;
    p.cols = (const int *)((const char *)m->dopt_tab.p + sbytes);
    p.A = m->dopt_scratch.as<double>();
    if ((rc = stage_one(m, m->st_aux2, prior, nn, mem, &p.prior))) return rc;
    // a host call's results of one chunk: [terms (4) | eig (n) | Cmat (n n)] per chunk, then the status words
    const size_t per_out = 4 + (eig ? n : 0) + (Cmat ? nn : 0);
    if (mem == FBR_HOST && (rc = m->dopt_out.ensure((size_t)ch * (per_out * sizeof(double) + sizeof(int))))) return rc;
    const unsigned threads = (unsigned)std::min<size_t>(256, 64 * ((n + 63) / 64));
    for (long c0 = 0; c0 < ngroups; c0 += ch) {
        const long cc = std::min<long>(ch, ngroups - c0);
        if ((rc = stage_one(m, m->st_aux, G + (size_t)c0 * gg, (size_t)cc * gg, mem, &p.G))) return rc;
        p.scale = scale ? (const double *)m->dopt_tab.p + c0 : nullptr;
        if (mem == FBR_HOST) {
            double *o = m->dopt_out.as<double>();
            p.terms = o;
            p.eig = eig ? o + 4 * (size_t)cc : nullptr;
            p.Cmat = Cmat ? o + (4 + (eig ? n : 0)) * (size_t)cc : nullptr;
            p.status = (int *)(o + per_out * (size_t)cc);
        } else {
            p.terms = terms + 4 * (size_t)c0;
            p.eig = eig ? eig + (size_t)c0 * n : nullptr;
            p.Cmat = Cmat ? Cmat + (size_t)c0 * nn : nullptr;
            p.status = status ? status + c0 : nullptr;
        }
        hipLaunchKernelGGL(fbr_dopt_kernel, dim3((unsigned)cc), dim3(threads), 0, m->stream, p);
        HIPCHK(hipGetLastError());
        if (mem == FBR_HOST) {
            HIPCHK(hipMemcpyAsync(terms + 4 * (size_t)c0, p.terms, (size_t)cc * 4 * sizeof(double), hipMemcpyDeviceToHost, m->stream));
            if (eig) HIPCHK(hipMemcpyAsync(eig + (size_t)c0 * n, p.eig, (size_t)cc * n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
            if (Cmat) HIPCHK(hipMemcpyAsync(Cmat + (size_t)c0 * nn, p.Cmat, (size_t)cc * nn * sizeof(double), hipMemcpyDeviceToHost, m->stream));
            if (status) HIPCHK(hipMemcpyAsync(status + c0, p.status, (size_t)cc * sizeof(int), hipMemcpyDeviceToHost, m->stream));
            HIPCHK(hipStreamSynchronize(m->stream));  // (the next chunk stages its Grams into the same buffers)
        }
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    return FBR_OK;
}

extern "C" int fbr_dopt_observability(fbr_model *m, const double *G, int32_t ngroups, int32_t Pa, const int32_t *cols, int32_t ncols,
                                      const double *prior, double threshold, int32_t *n_observable, double *energy, double *margin, double *eig,
                                      double *vec, int32_t *status, int32_t mem)
{
    if (int rc_check = dopt_check("fbr_dopt_observability", m, G, ngroups, Pa, cols, ncols, energy, "energy", mem)) return rc_check;
    if (!n_observable) {
        set_err("fbr_dopt_observability: n_observable is NULL");
        return FBR_E_INVALID;
    }
    if (!(threshold > 0.0) || !(threshold < 1.0)) {
        set_err("fbr_dopt_observability: threshold is not in (0, 1)");
        return FBR_E_INVALID;
    }
    if (threshold * threshold < 8.0 * fbr_dopt_band(ncols)) {
        char buf[256];
        snprintf(buf, sizeof buf, "fbr_dopt_observability: threshold %.3g is below what the Gram decides for %d columns: threshold^2 >= 8 band, band = %.3g "
                 "(fp64 knows an eigenvalue of the Gram to about band lambda_max)", threshold, (int)ncols, fbr_dopt_band(ncols));
        set_err(buf);
        return FBR_E_INVALID;
    }
    if (int rc_enter = enter_blocking(m)) return rc_enter;
    int rc;
    const size_t n = (size_t)ncols, nn = n * n, gg = (size_t)Pa * Pa;
    if ((rc = m->dopt_tab.ensure(n * sizeof(int)))) return rc;
    HIPCHK(hipMemcpyAsync(m->dopt_tab.p, cols, n * sizeof(int), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));  // (cols is the caller's)
    // candidates per launch: as fbr_dopt_terms, with 2 n^2 doubles of scratch each (A with the reflectors, the eigenvectors)
    long ch = std::min<long>(65535, std::max<long>(1, (long)(((size_t)256 << 20) / (2 * nn * sizeof(double)))));
    if (mem == FBR_HOST) ch = std::min<long>(ch, std::max<long>(1, (long)(((size_t)1 << 30) / (gg * sizeof(double)))));
    ch = std::min<long>(ch, ngroups);
    if ((rc = m->dopt_scratch.ensure((size_t)ch * 2 * nn * sizeof(double)))) return rc;
    DevDoptObs p;
    p.Pa = Pa, p.n = ncols, p.thr = threshold;
    p.cols = (const int *)m->dopt_tab.p;
    p.A = m->dopt_scratch.as<double>();
    if ((rc = stage_one(m, m->st_aux2, prior, nn, mem, &p.prior))) return rc;
    // a host call's results of one chunk: [energy (n) | margin (1) | eig (n) | vec (n n)] per chunk, then n_observable and the status words
    const size_t per_out = n + 1 + (eig ? n : 0) + (vec ? nn : 0);
    if (mem == FBR_HOST && (rc = m->dopt_out.ensure((size_t)ch * (per_out * sizeof(double) + 2 * sizeof(int))))) return rc;
    const unsigned threads = (unsigned)std::min<size_t>(256, 64 * ((n + 63) / 64));
    for (long c0 = 0; c0 < ngroups; c0 += ch) {
        const long cc = std::min<long>(ch, ngroups - c0);
        if ((rc = stage_one(m, m->st_aux, G + (size_t)c0 * gg, (size_t)cc * gg, mem, &p.G))) return rc;
        if (mem == FBR_HOST) {
            double *o = m->dopt_out.as<double>();
            p.energy = o;
            p.margin = o + n * (size_t)cc;
            p.eig = eig ? o + (n + 1) * (size_t)cc : nullptr;
            p.vec = vec ? o + (n + 1 + (eig ? n : 0)) * (size_t)cc : nullptr;
            p.n_observable = (int *)(o + per_out * (size_t)cc);
            p.status = p.n_observable + cc;
        } else {
            p.energy = energy + (size_t)c0 * n;
            p.margin = margin ? margin + c0 : nullptr;
            p.eig = eig ? eig + (size_t)c0 * n : nullptr;
            p.vec = vec ? vec + (size_t)c0 * nn : nullptr;
            p.n_observable = n_observable + c0;
            p.status = status ? status + c0 : nullptr;
        }
        hipLaunchKernelGGL(fbr_dopt_obs_kernel, dim3((unsigned)cc), dim3(threads), 0, m->stream, p);
        HIPCHK(hipGetLastError());
        if (mem == FBR_HOST) {
            HIPCHK(hipMemcpyAsync(energy + (size_t)c0 * n, p.energy, (size_t)cc * n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
            if (margin) HIPCHK(hipMemcpyAsync(margin + c0, p.margin, (size_t)cc * sizeof(double), hipMemcpyDeviceToHost, m->stream));
            if (eig) HIPCHK(hipMemcpyAsync(eig + (size_t)c0 * n, p.eig, (size_t)cc * n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
            if (vec) HIPCHK(hipMemcpyAsync(vec + (size_t)c0 * nn, p.vec, (size_t)cc * nn * sizeof(double), hipMemcpyDeviceToHost, m->stream));
            HIPCHK(hipMemcpyAsync(n_observable + c0, p.n_observable, (size_t)cc * sizeof(int), hipMemcpyDeviceToHost, m->stream));
            if (status) HIPCHK(hipMemcpyAsync(status + c0, p.status, (size_t)cc * sizeof(int), hipMemcpyDeviceToHost, m->stream));
            HIPCHK(hipStreamSynchronize(m->stream));  // (the next chunk stages its Grams into the same buffers)
        }
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    return FBR_OK;
}
