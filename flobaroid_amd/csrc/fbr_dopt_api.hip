// fbr_dopt_api.hip -- fbr_dopt_terms: eigenvalues, D-optimality terms and weight matrices of candidate Grams (kernel text: fbr_dopt.h).
#include "fbr_internal.h"
#include "fbr_dopt.h"

extern "C" int fbr_dopt_terms(fbr_model *m, const double *G, int32_t ngroups, int32_t Pa, const int32_t *cols, int32_t ncols, const double *prior,
                              double reg, const double *scale, double *terms, int32_t *status, double *eig, double *Cmat, int32_t mem)
{
    if (ngroups < 1) {
        set_err("fbr_dopt_terms: ngroups < 1");
        return FBR_E_INVALID;
    }
    if (!m || !G || !cols || !terms || (mem != FBR_HOST && mem != FBR_DEVICE)) {
        set_err("fbr_dopt_terms: m / G / cols / terms is NULL or a bad memory space");
        return FBR_E_INVALID;
    }
    if (ncols < 1 || ncols > Pa) {
        set_err("fbr_dopt_terms: ncols outside 1 .. Pa");
        return FBR_E_INVALID;
    }
    if (ncols > FBR_MAX_DOPT_COLUMNS) {
        set_err("fbr_dopt_terms: " + std::to_string(ncols) + " columns, more than FBR_MAX_DOPT_COLUMNS = " + std::to_string(FBR_MAX_DOPT_COLUMNS));
        return FBR_E_INVALID;
    }
    {
        std::vector<char> seen(Pa, 0);
        for (int i = 0; i < ncols; i++) {
            if (cols[i] < 0 || cols[i] >= Pa || seen[cols[i]]) {
                set_err("fbr_dopt_terms: cols holds an index out of range or twice");
                return FBR_E_INVALID;
            }
            seen[cols[i]] = 1;
        }
    }
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
