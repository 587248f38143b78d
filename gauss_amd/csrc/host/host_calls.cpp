// libgauss_host.so -- the one-call entry points of include/gauss_host.h: the drivers computeLD.cpp:26-166, dist.cpp:30-126,
// distmix.cpp:30-135, qcat.cpp / qcatmix.cpp, prep_qcat.cpp, zmix.cpp:201-1076, jepeg.cpp:28-153, jepegmix.cpp:26-161 with the numeric
// hot path delegated to libgauss_hip.so.
#include "host_internal.h"
#include <functional>


// Row store of a call on a packed panel: the resident copy in HBM when there is one, else -- the genotype section is small enough to
// make resident on the spot (a chromosome of the 33KG panel is 0.85 GB) -- uploaded now, else the mmap'd rows, gathered while
// staging.  An upload that fails leaves the mapped rows too.  The wait after panel_make_resident is kept for every caller: the
// upload it starts itself is synchronous, but it may instead FIND the entry of a background upload that a chromosome call on
// another thread started after panel_is_resident looked, and rows may only be read once they have landed (gauss_store_wait costs a
// map lookup when there is nothing to wait for, and this branch runs once per panel and context).
static const int64_t RESIDENT_ON_DEMAND_MAX_BYTES = (int64_t)4 << 30;
static void panel_rows(gauss_ctx* ctx, const std::string& path, const PackedPanel& pk, const uint8_t** store, int* on_device)
{
    void* dev = nullptr;
    const bool resident = panel_is_resident(ctx, path, &dev) ||
                          (pk.n_snp() * pk.row_bytes() <= RESIDENT_ON_DEMAND_MAX_BYTES && panel_make_resident(ctx, path, &dev, nullptr) == 0 &&
                           gauss_store_wait(ctx, dev, 0) == 0);
    *store = resident ? (const uint8_t*)dev : pk.geno();
    *on_device = resident ? 1 : 0;
}

// The arguments every one-window call shares, filled once per entry point: call_pop for the study_pop form, call_mix for the
// pop_names / pop_wgts / n form
struct CallArgs {
    int kind, chr;
    int64_t start_bp, end_bp, wing;
    const char* study_pop;
    const char* const* pop_names; const double* pop_wgts; int n_pop_wgt;
    const char *input, *index, *data, *desc;
    double af1_cutoff;
};
static CallArgs call_mix(int kind, int chr, int64_t start_bp, int64_t end_bp, int64_t wing, const char* const* pop_names, const double* pop_wgts,
                         int n_pop_wgt, const char* input, const char* index, const char* data, const char* desc, double af1_cutoff)
{
    return {kind, chr, start_bp, end_bp, wing, nullptr, pop_names, pop_wgts, n_pop_wgt, input, index, data, desc, af1_cutoff};
}
static CallArgs call_pop(int kind, int chr, int64_t start_bp, int64_t end_bp, int64_t wing, const char* study_pop, const char* input,
                         const char* index, const char* data, const char* desc, double af1_cutoff)
{
    return {kind, chr, start_bp, end_bp, wing, study_pop, nullptr, nullptr, 0, input, index, data, desc, af1_cutoff};
}

// ... and of a gene call: no window, and both forms (the rank entry points take either): the kind says which one is read
static CallArgs call_gene(int kind, const char* study_pop, const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input,
                          const char* index, const char* data, const char* desc, double af1_cutoff)
{
    return {kind, 0, 0, 0, 0, study_pop, pop_names, pop_wgts, n_pop_wgt, input, index, data, desc, af1_cutoff};
}

static bool mix_kind(int kind)                               // the kinds that read pop_names / pop_wgts, not study_pop
{
    return kind == GAUSS_KIND_COMPUTELD || kind == GAUSS_KIND_DISTMIX || kind == GAUSS_KIND_JEPEGMIX || kind == GAUSS_KIND_QCATMIX ||
           kind == GAUSS_KIND_PREP_RECESSIVE || kind == GAUSS_KIND_LDSCOREMIX;
}

// gauss_host_prepare on a panel that open_panel has resolved already (panel_path, pk: empty for a text panel)
static int prepare_opened(const CallArgs& c, const char* annotation_file, const std::string& panel_path, const std::shared_ptr<PackedPanel>& pk,
                          bool annotated_only, gauss_prepared** out)
{
    const int kind = c.kind;
    std::unique_ptr<gauss_prepared> p(new gauss_prepared());
    p->kind = kind;
    Args& a = p->args;
    a.chr = c.chr; a.start_bp = c.start_bp; a.end_bp = c.end_bp;
    a.wing_size = (kind == GAUSS_KIND_COMPUTELD) ? 0 : c.wing;          // computeLD.cpp:40
    if (c.study_pop) a.study_pop = c.study_pop;
    a.input_file = c.input; a.reference_index_file = c.index;
    a.reference_data_file = panel_path; a.reference_pop_desc_file = c.desc;
    if (annotation_file) a.annotation_file = annotation_file;
    a.pk = pk;
    a.drop_wing_unmeasured = pk && (kind == GAUSS_KIND_DIST || kind == GAUSS_KIND_DISTMIX);
    a.af1_cutoff = std::isnan(c.af1_cutoff) ? (kind == GAUSS_KIND_QCAT ? 0.05 : 0.01) : c.af1_cutoff;   // dist.cpp:53-57, qcat.cpp:53-57
    if (mix_kind(kind)) {
        if (!c.pop_names || !c.pop_wgts || c.n_pop_wgt < 1) return herr("pop_wgt_df is empty");
        set_pop_wgt_map(a, c.pop_names, c.pop_wgts, c.n_pop_wgt);
    } else if (!c.study_pop) return herr("study_pop is NULL");
    if ((kind == GAUSS_KIND_JEPEG || kind == GAUSS_KIND_JEPEGMIX) && !annotation_file) return herr("annotation_file is NULL");
    a.annotated_only = annotated_only && (kind == GAUSS_KIND_JEPEG || kind == GAUSS_KIND_JEPEGMIX);
    if (prepare(*p)) return -1;
    *out = p.release();
    return 0;
}

// annotated_only: the gene drivers' SNP map (run_jepeg); gauss_host_prepare enters the whole study, as the reference does
// (gauss_prepared_snps lists it)
static int prepare_files(const CallArgs& c, const char* annotation_file, bool annotated_only, gauss_prepared** out)
{
    if (!out) return herr("out is NULL");
    if (c.kind < 0 || c.kind > GAUSS_KIND_PREP_RECESSIVE) return herr("bad kind %d", c.kind);
    if (files_ok({c.input, c.index, c.data, c.desc})) return -1;
    std::string panel_path;
    std::shared_ptr<PackedPanel> pk;
    if (open_panel(c.index, c.data, c.desc, panel_path, pk)) return -1;
    return prepare_opened(c, annotation_file, panel_path, pk, annotated_only, out);
}

extern "C" {

int gauss_host_prepare(int kind, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                       const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                       const char* annotation_file, const char* reference_index_file, const char* reference_data_file,
                       const char* reference_pop_desc_file, double af1_cutoff, gauss_prepared** out)
{
    CallArgs c = call_mix(kind, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file, reference_index_file,
                          reference_data_file, reference_pop_desc_file, af1_cutoff);
    c.study_pop = study_pop;                                 // this entry point takes both forms: the kind says which one is read
    return prepare_files(c, annotation_file, false, out);
}

const gauss_table* gauss_prepared_snps(const gauss_prepared* p)
{
    if (!p) return nullptr;
    if (!p->snps_built) build_snp_table(*const_cast<gauss_prepared*>(p));      // a debugging / test view: built on demand
    return &p->snps;
}
int gauss_prepared_counts(const gauss_prepared* p, int* m, int* u, int* n, int* np, int* ng)
{
    if (!p) return herr("prepared is NULL");
    if (m) *m = (int)p->measured.size();
    if (u) *u = (int)p->unmeasured.size();
    if (n) *n = p->N;
    if (np) *np = (int)p->pop_off.size() - 1;
    if (ng) *ng = p->gene_off.empty() ? 0 : (int)p->gene_off.size() - 1;
    return 0;
}
const int32_t* gauss_prepared_measured_rows(const gauss_prepared* p) { return p ? p->measured_rows.data() : nullptr; }
const int32_t* gauss_prepared_unmeasured_rows(const gauss_prepared* p) { return p ? p->unmeasured_rows.data() : nullptr; }
static void ensure_bytes(const gauss_prepared* cp)
{
    gauss_prepared* p = const_cast<gauss_prepared*>(cp);     // lazily unpacked view of packed rows (tests, debugging)
    if (p->packed_rows && p->gm.empty()) materialise_from_packed(*p);
}
const uint8_t* gauss_prepared_geno_m(const gauss_prepared* p, int64_t* ld) { if (!p) return nullptr; ensure_bytes(p); if (ld) *ld = p->ld; return p->gm.data(); }
const uint8_t* gauss_prepared_geno_u(const gauss_prepared* p, int64_t* ld) { if (!p) return nullptr; ensure_bytes(p); if (ld) *ld = p->ld; return p->gu.data(); }
int gauss_prepared_packed_store(const gauss_prepared* p, const uint8_t** base, int64_t* bytes, int64_t* row_bytes)
{
    if (!p) return herr("prepared is NULL");
    if (!p->packed_rows) { if (base) *base = nullptr; if (bytes) *bytes = 0; if (row_bytes) *row_bytes = 0; return 0; }
    const PackedPanel& pk = *p->args.pk;
    if (base) *base = pk.geno();
    if (bytes) *bytes = pk.n_snp() * pk.row_bytes();
    if (row_bytes) *row_bytes = pk.row_bytes();
    return 0;
}
const int32_t* gauss_prepared_pop_off(const gauss_prepared* p) { return p ? p->pop_off.data() : nullptr; }
const double* gauss_prepared_pop_wgt(const gauss_prepared* p) { return p ? p->pop_wgt.data() : nullptr; }
const double* gauss_prepared_z1(const gauss_prepared* p) { return p ? p->z1.data() : nullptr; }
const int32_t* gauss_prepared_gene_off(const gauss_prepared* p) { return (p && !p->gene_off.empty()) ? p->gene_off.data() : nullptr; }
void gauss_prepared_free(gauss_prepared* p) { delete p; }

int gauss_prepared_qcat_counts(const gauss_prepared* p, int* n_head, int* n_predm)
{
    if (!p) return herr("prepared is NULL");
    if (n_head) *n_head = p->n_head;
    if (n_predm) *n_predm = p->n_predm;
    return 0;
}

// populations and genotype source of a prepared window: host byte matrices, or row lists into the mmap'd packed panel
static void prepared_source(const gauss_prepared& p, gauss_window_desc& d)
{
    d.n_pop = (int)p.pop_off.size() - 1;
    d.pop_off = p.pop_off.data(); d.pop_wgt = p.pop_wgt.data();
    if (!p.packed_rows) { d.geno_m = p.gm.data(); d.geno_u = p.gu.data(); d.ld = p.ld; return; }
    const PackedPanel& pk = *p.args.pk;
    d.geno_format = GAUSS_GENO_2BIT;
    d.geno_m = d.geno_u = pk.geno();
    d.ld = pk.row_bytes();
    d.rows_m = p.store_rows_m.data();
    d.rows_u = p.store_rows_u.data();
    d.pop_src_off = p.pop_src_off.data();
}

int gauss_prepared_window_desc(gauss_prepared* p, gauss_window_desc* d)
{
    if (!p || !d) return herr("bad arguments");
    const bool qcat = (p->kind == GAUSS_KIND_QCAT || p->kind == GAUSS_KIND_QCATMIX);
    const bool prep = (p->kind == GAUSS_KIND_PREP_QCAT || p->kind == GAUSS_KIND_PREP_RECESSIVE);
    if (p->kind != GAUSS_KIND_DIST && p->kind != GAUSS_KIND_DISTMIX && !qcat && !prep) return herr("not a window kind");
    const Args& a = p->args;
    const int M = (int)p->measured.size(), U = (int)p->unmeasured.size();
    if (prep) {
        if (M <= a.min_num_measured_snp)                       // prep_qcat.cpp:86-91, prep_qcatmix.cpp:126-128
            return herr("Not enough number of SNPs loaded - %s not performed (measured %d, prediction window %d)",
                        p->kind == GAUSS_KIND_PREP_QCAT ? "QCAT" : "Recessive Imputation", M, U);
        const int ncode = (p->kind == GAUSS_KIND_PREP_RECESSIVE) ? 3 : 1;
        p->out_b11.assign((size_t)M * M, 0.0);
        p->out_b21.assign((size_t)std::max(1, ncode * U) * M, 0.0);
        memset(d, 0, sizeof(*d));
        d->kind = GAUSS_WIN_LD;
        d->mode = (p->kind == GAUSS_KIND_PREP_QCAT) ? GAUSS_MODE_POOLED : GAUSS_MODE_WEIGHTED;
        d->n_measured = M; d->n_unmeasured = U;
        prepared_source(*p, *d);
        d->lambda = 0.0;                                       // B11(i,i) = 1.0 (prep_qcat.cpp:109)
        d->u_codings = (ncode == 3) ? (GAUSS_CODE_ADDITIVE | GAUSS_CODE_DOMINANT | GAUSS_CODE_RECESSIVE) : GAUSS_CODE_ADDITIVE;
        d->out_b11 = p->out_b11.data(); d->out_b21 = p->out_b21.data(); d->out_status = &p->status;
        return 0;
    }
    if (qcat) {
        // qcat.cpp:157-162 guards on the measured count only; qcatmix.cpp:168-174 on both (texts as in the reference)
        if (p->kind == GAUSS_KIND_QCAT && M <= a.min_num_measured_snp)
            return herr("Not enough number of SNPs loaded - QCAT not performed (measured %d, unmeasured %d)", M, U);
        if (p->kind == GAUSS_KIND_QCATMIX && (M <= a.min_num_measured_snp || U <= a.min_num_unmeasured_snp))
            return herr("Not enough number of SNPs loaded - QCAT performed (measured %d, unmeasured %d)", M, U);
        p->out_r.assign((size_t)p->n_predm + U, 0.0);
        p->num_eig = M;
        memset(d, 0, sizeof(*d));
        d->kind = GAUSS_WIN_QCAT;
        d->mode = (p->kind == GAUSS_KIND_QCAT) ? GAUSS_MODE_POOLED : GAUSS_MODE_WEIGHTED;
        d->n_measured = M; d->n_unmeasured = U;
        prepared_source(*p, *d);
        d->z1 = p->z1.data(); d->lambda = a.lambda; d->min_abs_eig = a.min_abs_eig;
        d->n_head_measured = p->n_head; d->n_pred_measured = p->n_predm; d->eig_cutoff = a.eig_cutoff;
        d->out_r = p->out_r.data(); d->out_num_eig = &p->num_eig; d->out_status = &p->status;
        if (p->n_predm + U < 1) return herr("QCAT window has no SNP to test");
        return 0;
    }
    if (M <= a.min_num_measured_snp || U <= a.min_num_unmeasured_snp)      // dist.cpp:145-151
        return herr("Not enough number of SNPs loaded - %s not performed (measured %d, unmeasured %d)",
                    p->kind == GAUSS_KIND_DIST ? "DIST" : "DISTMIX", M, U);
    p->out_z.assign(U, 0.0); p->out_info.assign(U, 0.0);
    memset(d, 0, sizeof(*d));
    d->mode = (p->kind == GAUSS_KIND_DIST) ? GAUSS_MODE_POOLED : GAUSS_MODE_WEIGHTED;
    d->n_measured = M; d->n_unmeasured = U;
    prepared_source(*p, *d);
    d->z1 = p->z1.data(); d->lambda = a.lambda; d->min_abs_eig = a.min_abs_eig;
    d->out_z = p->out_z.data(); d->out_info = p->out_info.data(); d->out_status = &p->status;
    return 0;
}

int gauss_prepared_finish(gauss_prepared* p, gauss_table** out)
{
    if (!p || !out) return herr("bad arguments");
    if (p->kind == GAUSS_KIND_PREP_QCAT || p->kind == GAUSS_KIND_PREP_RECESSIVE) { *out = prep_output(*p); return 0; }
    if (p->kind == GAUSS_KIND_QCAT || p->kind == GAUSS_KIND_QCATMIX) {
        const int m = p->num_eig;
        for (size_t t = 0; t < p->out_r.size(); t++) {                           // qcat.cpp:216-243
            Snp* s = (t < (size_t)p->n_predm) ? p->measured[p->n_head + t] : p->unmeasured[t - p->n_predm];
            const double r = p->out_r[t];
            s->qcat_m = m;
            s->qcat_t = std::sqrt((double)(m - 3)) * r;
            s->qcat_chisq = (m - 3) * r * r;
        }
        *out = qcat_output(*p);
        return 0;
    }
    for (size_t i = 0; i < p->unmeasured.size() && i < p->out_z.size(); i++) {   // dist.cpp:200-202
        p->unmeasured[i]->z = p->out_z[i];
        p->unmeasured[i]->info = p->out_info[i];
    }
    *out = dist_output(*p);
    return 0;
}

// dist() / distmix() / qcat() / qcatmix(): ONE window per call, the reference's own usage (docs/articles/dist_example.md:144-153).
//
// CallWindow is the window of such a call, and the one place that knows which of two ways it was built:
//   lean     on a sorted packed panel, as the chromosome driver builds its windows (host_chrom.cpp: LeanWindow -- a merge of the
//            study's rows and the panel's SNP table instead of per-SNP objects in a map: ~0.1 ms against 0.7-1.0).  Its genotype rows
//            are read from the panel's resident copy in HBM (panel_rows) instead of being gathered on the host and copied per call
//            (24 MB a window), and it runs as a job on those rows.  Measured on the chr22 study, window after window
//            (tools/window_calls_probe.py): 5.9 ms per call -> 2.5.
//   literal  for an unsorted or text panel, a call over every chromosome, GAUSS_HOST_FULL_MAP=1 or a kind the lean window does not
//            build: prepare() into a gauss_prepared, rows on the host.
// Callers read it through the members.  It stays where it was built (w points into cs; the view and the descriptors point into it).
struct CallWindow {
    // errors come in prepare()'s order: arguments, description file, populations, study file
    int build(const CallArgs& c, const std::string& panel_path, const std::shared_ptr<PackedPanel>& pk, bool lean_allowed = true);
    bool lean() const { return !prep; }
    const Args& args() const { return prep ? prep->args : cs.a; }
    size_t n_measured() const { return prep ? prep->measured.size() : w.measured.size(); }
    size_t n_unmeasured() const { return prep ? prep->unmeasured.size() : w.unmeasured.size(); }
    ViewSnp measured(size_t i) const { return prep ? snp(*prep->measured[i]) : snp(w.v[(size_t)w.measured[i]]); }       // matrix row order
    ViewSnp unmeasured(size_t i) const { return prep ? snp(*prep->unmeasured[i]) : snp(w.v[(size_t)w.unmeasured[i]]); }
    void source(gauss_window_desc& d) const;            // populations, genotype format and rows; a lean window's geno_m / geno_u are run()'s
    int desc(gauss_window_desc* d) { return prep ? gauss_prepared_window_desc(prep.get(), d) : lean_window_desc(w, d); }
    int plain(gauss_table** t);                         // the call's own table: gauss_prepared_finish | lean_window_finish
    WindowView view();                                  // what a rider reads; built only when asked for
    int run(gauss_ctx* ctx, gauss_window_desc* d, int n = 1) const;
    std::unique_ptr<gauss_prepared> release() { return std::move(prep); }      // a literal window's host rows, for who outlives it (LdRows)

private:
    CallArgs c;
    bool mix = false;
    std::string path;
    std::shared_ptr<PackedPanel> pk;
    ChromSetup cs;
    LeanWindow w;
    std::unique_ptr<gauss_prepared> prep;
    int wing_of(long long bp) const { const int ibp = (int)bp; return ibp >= c.start_bp && ibp <= c.end_bp ? 0 : 1; }      // dist.cpp:92
    ViewSnp snp(const Snp& s) const { return {ident_of(s), mix ? s.af1mix : s.af1ref, s.z, wing_of(s.bp)}; }
    ViewSnp snp(const LeanSnp& sn) const { return {ident_of(*pk, sn), sn.af, sn.z, wing_of(sn.bp)}; }
};

int CallWindow::build(const CallArgs& c_, const std::string& panel_path, const std::shared_ptr<PackedPanel>& pk_, bool lean_allowed)
{
    c = c_; mix = mix_kind(c.kind); path = panel_path; pk = pk_;
    if (lean_allowed && c.chr > 0 && !env_flag("GAUSS_HOST_FULL_MAP", false) && pk && pk->header().sorted) {
        if (chrom_setup(cs, c.kind, c.chr, c.wing, c.study_pop, c.pop_names, c.pop_wgts, c.n_pop_wgt, c.input, path, c.desc, c.af1_cutoff, pk,
                        nullptr)) return -1;
        std::string err;
        cs.gw = load_gwas_cached(c.input, err);
        if (!cs.gw) return herr("%s", err.c_str());
        return lean_window_build(w, cs, c.start_bp, c.end_bp) ? -1 : 0;
    }
    gauss_prepared* p = nullptr;
    if (prepare_opened(c, nullptr, path, pk, false, &p)) return -1;
    prep.reset(p);
    return 0;
}

void CallWindow::source(gauss_window_desc& d) const
{
    if (prep) return prepared_source(*prep, d);
    d.n_pop = (int)cs.pop_off.size() - 1;
    d.pop_off = cs.pop_off.data(); d.pop_wgt = cs.pop_wgt.data();
    d.geno_format = GAUSS_GENO_2BIT;
    d.ld = pk->row_bytes();
    d.rows_m = w.store_rows_m.data(); d.rows_u = w.store_rows_u.data();
    d.pop_src_off = cs.pop_src_off.data();
}

int CallWindow::plain(gauss_table** t)
{
    if (prep) return gauss_prepared_finish(prep.get(), t);
    *t = lean_window_finish(w);
    return 0;
}

WindowView CallWindow::view()
{
    WindowView v;
    v.mix = mix;
    v.plain = [this](gauss_table** t) { return plain(t); };
    // the rows of the plain table: the SNPs of the prediction window, snp_vec order (dist_output; lean_table_count fills out_row)
    std::map<const Snp*, int32_t> row_of;
    if (prep) { for (const Snp* sn : prep->snp_vec) if (!wing_of(sn->bp)) { const int32_t r = (int32_t)row_of.size(); row_of[sn] = r; } }
    else lean_table_count(w);
    auto row = [&](bool m, size_t i) {
        if (!prep) return w.out_row[(size_t)(m ? w.measured : w.unmeasured)[i]];
        auto it = row_of.find((m ? prep->measured : prep->unmeasured)[i]);
        return it == row_of.end() ? -1 : it->second;
    };
    for (size_t i = 0; i < n_measured(); i++) { v.measured.push_back(measured(i)); v.row_m.push_back(row(true, i)); }
    for (size_t i = 0; i < n_unmeasured(); i++) v.row_u.push_back(row(false, i));
    return v;
}

// d[0 .. n): this window's descriptor, then those of its peers, built the same way on the same panel (run_xsusie).  Lean windows run
// on the rows panel_rows names -- as a job on the resident panel, or, for a panel too large to keep in HBM, on the rows of the
// mapped file; literal ones on the rows their descriptors already name.  One window off the device is gauss_impute_window.
int CallWindow::run(gauss_ctx* ctx, gauss_window_desc* d, int n) const
{
    int on_device = 0;
    if (!prep) {
        const uint8_t* store = nullptr;
        panel_rows(ctx, path, *pk, &store, &on_device);
        for (int k = 0; k < n; k++) d[k].geno_m = d[k].geno_u = store;
    }
    int rc;
    if (on_device || n > 1) {
        gauss_job* job = nullptr;
        rc = gauss_job_create(ctx, d, n, on_device, &job);
        if (rc == 0) rc = gauss_job_run(job);
        if (rc == 0) rc = gauss_job_fetch(job);
        if (job) gauss_job_destroy(job);
    } else rc = gauss_impute_window(ctx, d);
    return rc ? herr("%s", gauss_last_error()) : 0;
}

// rider: what the call asks beyond its plain table (host_internal.h: Rider), or NULL.  The view is built only for a rider: a
// plain call does not pay for it.
static int run_impute(gauss_ctx* ctx, const CallArgs& c, Rider* rider, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    if (files_ok({c.input, c.index, c.data, c.desc})) return -1;
    if (rider && rider->check()) return -1;
    std::string panel_path;
    std::shared_ptr<PackedPanel> pk;
    if (open_panel(c.index, c.data, c.desc, panel_path, pk)) return -1;
    CallWindow win;                                           // (the descriptor and the view point into it)
    if (win.build(c, panel_path, pk, c.kind != GAUSS_KIND_PREP_QCAT && c.kind != GAUSS_KIND_PREP_RECESSIVE)) return -1;
    gauss_window_desc d;
    if (win.desc(&d)) return -1;
    if (!rider) return win.run(ctx, &d) ? -1 : win.plain(out);
    WindowView v = win.view();
    if (rider->ask(d, v)) return -1;
    if (win.run(ctx, &d)) return -1;
    return rider->table(v, out);
}

int gauss_host_dist(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                    const char* input_file, const char* reference_index_file, const char* reference_data_file,
                    const char* reference_pop_desc_file, double af1_cutoff, gauss_table** out)
{
    return run_impute(ctx, call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), nullptr, out);
}

int gauss_host_distmix(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                       const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                       const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                       double af1_cutoff, gauss_table** out)
{
    return run_impute(ctx, call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), nullptr, out);
}

int gauss_host_dist_loo(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                        const char* input_file, const char* reference_index_file, const char* reference_data_file,
                        const char* reference_pop_desc_file, double af1_cutoff, gauss_table** out)
{
    LooRider r;
    return run_impute(ctx, call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_distmix_loo(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                           const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                           const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                           double af1_cutoff, gauss_table** out)
{
    LooRider r;
    return run_impute(ctx, call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_dist_slct(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                         const char* input_file, const char* reference_index_file, const char* reference_data_file,
                         const char* reference_pop_desc_file, double af1_cutoff, double p_cutoff, double collin, int max_signals,
                         const char* const* cond_rsids, int n_cond, gauss_table** out)
{
    SlctRider r(p_cutoff, collin, max_signals, cond_rsids, n_cond, false);
    return run_impute(ctx, call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_distmix_slct(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                            const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                            const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                            double af1_cutoff, double p_cutoff, double collin, int max_signals,
                            const char* const* cond_rsids, int n_cond, gauss_table** out)
{
    SlctRider r(p_cutoff, collin, max_signals, cond_rsids, n_cond, false);
    return run_impute(ctx, call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_dist_cond(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                         const char* input_file, const char* reference_index_file, const char* reference_data_file,
                         const char* reference_pop_desc_file, double af1_cutoff, double p_cutoff, double collin, int max_signals,
                         const char* const* cond_rsids, int n_cond, gauss_table** out)
{
    SlctRider r(p_cutoff, collin, max_signals, cond_rsids, n_cond, true);
    return run_impute(ctx, call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_distmix_cond(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                            const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                            const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                            double af1_cutoff, double p_cutoff, double collin, int max_signals,
                            const char* const* cond_rsids, int n_cond, gauss_table** out)
{
    SlctRider r(p_cutoff, collin, max_signals, cond_rsids, n_cond, true);
    return run_impute(ctx, call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_dist_cs(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                       const char* input_file, const char* reference_index_file, const char* reference_data_file,
                       const char* reference_pop_desc_file, double af1_cutoff, double p_cutoff, double collin, int max_signals,
                       const char* const* cond_rsids, int n_cond, double coverage, double prior_var, gauss_table** out)
{
    CsRider r(p_cutoff, collin, max_signals, cond_rsids, n_cond, coverage, prior_var);
    return run_impute(ctx, call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_distmix_cs(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                          const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                          const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                          double af1_cutoff, double p_cutoff, double collin, int max_signals,
                          const char* const* cond_rsids, int n_cond, double coverage, double prior_var, gauss_table** out)
{
    CsRider r(p_cutoff, collin, max_signals, cond_rsids, n_cond, coverage, prior_var);
    return run_impute(ctx, call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_dist_susie(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                          const char* input_file, const char* reference_index_file, const char* reference_data_file,
                          const char* reference_pop_desc_file, double af1_cutoff, int L, double coverage, double prior_var,
                          double min_abs_corr, int max_sweeps, double tol, int estimate_prior_var, int measured_only, gauss_table** out)
{
    SusieRider r(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only);
    return run_impute(ctx, call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_distmix_susie(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                             const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                             const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                             double af1_cutoff, int L, double coverage, double prior_var, double min_abs_corr, int max_sweeps, double tol,
                             int estimate_prior_var, int measured_only, gauss_table** out)
{
    SusieRider r(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only);
    return run_impute(ctx, call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

// dist_xsusie / distmix_xsusie: K studies of one trait on one panel, fitted jointly (gauss_window_desc.xs_group).  Every study's window
// is built exactly as its own dist() / distmix() call builds it (run_impute), the maps come from the panel SNP each candidate is
// (xs_build_map), and the K windows run as one job.  The table is study 1's *_susie table with the joint values (xsusie_output).
struct XsStudy {
    CallWindow win;                      // (built in place, never moved)
    WindowView v;
    std::vector<int64_t> key;            // the panel SNP of every candidate, measured first
    std::vector<int32_t> from_lead;
};
static int run_xsusie(gauss_ctx* ctx, const std::vector<CallArgs>& calls, SusieRider& r, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    const int K = (int)calls.size();
    if (K < 2 || K > GAUSS_XS_MAX) return herr("n_studies = %d: the joint fit takes 2 .. %d studies", K, GAUSS_XS_MAX);
    for (const CallArgs& c : calls) if (files_ok({c.input, c.index, c.data, c.desc})) return -1;
    if (r.check()) return -1;
    const CallArgs& c0 = calls[0];
    std::string panel_path;
    std::shared_ptr<PackedPanel> pk;
    if (open_panel(c0.index, c0.data, c0.desc, panel_path, pk)) return -1;
    std::vector<std::unique_ptr<XsStudy>> st;
    std::vector<gauss_window_desc> d((size_t)K);
    std::vector<int32_t> status((size_t)K, 0);
    std::map<std::string, int64_t> snp_no;                                  // chr:bp:rsid -> one number per panel SNP
    auto key_of = [&](const SnpIdent& id) {
        const std::string s = std::to_string(id.chr) + ":" + std::to_string(id.bp) + ":" + (id.rsid ? id.rsid : "");
        return snp_no.emplace(s, (int64_t)snp_no.size()).first->second;
    };
    for (int k = 0; k < K; k++) {
        st.emplace_back(new XsStudy());
        XsStudy& s = *st.back();
        if (s.win.build(calls[(size_t)k], panel_path, pk)) return -1;
        if (s.win.lean() != st[0]->win.lean()) return herr("study %d cannot be built the way study 1 is", k + 1);
        if (s.win.desc(&d[(size_t)k])) return -1;
        s.v = s.win.view();
        for (const ViewSnp& m : s.v.measured) s.key.push_back(key_of(m.id));
        for (size_t i = 0; i < s.win.n_unmeasured(); i++) s.key.push_back(key_of(s.win.unmeasured(i).id));
        d[(size_t)k].out_status = &status[(size_t)k];
    }
    // the leader asks for the fit; the peers take its arguments and their maps
    if (r.ask(d[0], st[0]->v)) return -1;
    const size_t TL = st[0]->key.size(), L = (size_t)r.n_eff;
    std::vector<double> xs_V((size_t)K * L, NAN), xs_purity((size_t)K * L, NAN);
    std::vector<uint8_t> joint(TL, 1);
    d[0].xs_group = 1; d[0].out_xs_V = xs_V.data(); d[0].out_xs_purity = xs_purity.data();
    for (int k = 1; k < K; k++) {
        XsStudy& s = *st[(size_t)k];
        gauss_window_desc& q = d[(size_t)k];
        q.susie_L = d[0].susie_L; q.susie_coverage = d[0].susie_coverage; q.susie_prior_var = d[0].susie_prior_var; q.susie_tol = d[0].susie_tol;
        q.susie_min_abs_corr = d[0].susie_min_abs_corr; q.susie_max_sweeps = d[0].susie_max_sweeps;
        q.susie_estimate_var = d[0].susie_estimate_var; q.susie_measured_only = d[0].susie_measured_only;
        s.from_lead.assign(TL, -1);
        if (xs_build_map(st[0]->key.data(), TL, s.key.data(), s.key.size(), s.from_lead.data()) < 0) return -1;
        for (size_t j = 0; j < TL; j++) if (s.from_lead[j] < 0) joint[j] = 0;
        q.xs_group = 1; q.xs_from_lead = s.from_lead.data();
    }
    if (st[0]->win.run(ctx, d.data(), K)) return -1;
    if (r.table(st[0]->v, out)) return -1;
    if (xsusie_output(**out, st[0]->v.row_m, st[0]->v.row_u, joint.data(), K, (int)L, xs_V.data(), xs_purity.data(), status.data())) {
        gauss_table_free(*out); *out = nullptr;
        return -1;
    }
    return 0;
}

int gauss_host_dist_xsusie(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* const* study_pops,
                           const char* const* input_files, int n_studies, const char* reference_index_file, const char* reference_data_file,
                           const char* reference_pop_desc_file, double af1_cutoff, int L, double coverage, double prior_var,
                           double min_abs_corr, int max_sweeps, double tol, int estimate_prior_var, int measured_only, gauss_table** out)
{
    if (!study_pops || !input_files) return herr("bad arguments");
    SusieRider r(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only);
    std::vector<CallArgs> calls;
    for (int k = 0; k < n_studies; k++)
        calls.push_back(call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pops[k], input_files[k], reference_index_file,
                                 reference_data_file, reference_pop_desc_file, af1_cutoff));
    return run_xsusie(ctx, calls, r, out);
}

int gauss_host_distmix_xsusie(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* const* pop_names,
                              const double* pop_wgts, int n_pop_wgt, const char* const* input_files, int n_studies,
                              const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                              double af1_cutoff, int L, double coverage, double prior_var, double min_abs_corr, int max_sweeps, double tol,
                              int estimate_prior_var, int measured_only, gauss_table** out)
{
    if (!pop_names || !pop_wgts || !input_files || n_pop_wgt < 1) return herr("bad arguments");
    SusieRider r(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only);
    std::vector<CallArgs> calls;
    for (int k = 0; k < n_studies; k++)                                    // pop_wgts [n_studies][n_pop_wgt]: study k's weights of the same names
        calls.push_back(call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts + (size_t)k * n_pop_wgt, n_pop_wgt,
                                 input_files[k], reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff));
    return run_xsusie(ctx, calls, r, out);
}

int gauss_host_dist_coloc(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                          const char* input_file, const char* reference_index_file, const char* reference_data_file,
                          const char* reference_pop_desc_file, double af1_cutoff, const char* const* more_input_files, int n_more, int L,
                          double coverage, double prior_var, double min_abs_corr, int max_sweeps, double tol, int estimate_prior_var,
                          int measured_only, double p1, double p2, double p12, gauss_table** out)
{
    ColocRider r(more_input_files, n_more, SusieRider(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only),
                 p1, p2, p12);
    return run_impute(ctx, call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_distmix_coloc(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                             const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                             const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                             double af1_cutoff, const char* const* more_input_files, int n_more, int L, double coverage, double prior_var,
                             double min_abs_corr, int max_sweeps, double tol, int estimate_prior_var, int measured_only, double p1, double p2,
                             double p12, gauss_table** out)
{
    ColocRider r(more_input_files, n_more, SusieRider(L, coverage, prior_var, min_abs_corr, max_sweeps, tol, estimate_prior_var, measured_only),
                 p1, p2, p12);
    return run_impute(ctx, call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_dist_prs(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                        const char* input_file, const char* reference_index_file, const char* reference_data_file,
                        const char* reference_pop_desc_file, double af1_cutoff, double n, const double* s, int n_s, const double* lam,
                        int n_lam, double tol, int max_sweeps, gauss_table** out)
{
    PrsRider r(n, s, n_s, lam, n_lam, tol, max_sweeps);
    return run_impute(ctx, call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_distmix_prs(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                           const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                           const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                           double af1_cutoff, double n, const double* s, int n_s, const double* lam, int n_lam, double tol, int max_sweeps,
                           gauss_table** out)
{
    PrsRider r(n, s, n_s, lam, n_lam, tol, max_sweeps);
    return run_impute(ctx, call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

// dist_ldscore / distmix_ldscore: ONE window of a kind of its own -- the targets are the study's SNPs inside [start_bp, end_bp], the
// reference rows every other panel SNP of the extended window (lean_window_build / prepare make the partition) -- run as an LD window
// that asks for its LD scores and for no matrix: M numbers come back (include/gauss_host.h)
static int run_ldscore(gauss_ctx* ctx, const CallArgs& c, double n_arg, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    if (files_ok({c.input, c.index, c.data, c.desc})) return -1;
    std::string panel_path;
    std::shared_ptr<PackedPanel> pk;
    if (open_panel(c.index, c.data, c.desc, panel_path, pk)) return -1;
    const bool mix = c.kind == GAUSS_KIND_LDSCOREMIX;
    CallWindow win;
    if (win.build(c, panel_path, pk)) return -1;
    std::vector<ViewSnp> rows;
    std::vector<int32_t> bp_m, bp_u;
    int64_t n_ref = 0, n_ref_5_50 = 0;
    auto count = [&](double af) { n_ref++; if (std::min(af, 1.0 - af) > 0.05) n_ref_5_50++; };
    for (size_t i = 0; i < win.n_measured(); i++) { rows.push_back(win.measured(i)); bp_m.push_back((int32_t)rows.back().id.bp); count(rows.back().af); }
    for (size_t i = 0; i < win.n_unmeasured(); i++) { const ViewSnp s = win.unmeasured(i); bp_u.push_back((int32_t)s.id.bp); count(s.af); }
    gauss_window_desc d;
    memset(&d, 0, sizeof(d));
    d.kind = GAUSS_WIN_LD;
    d.mode = mix ? GAUSS_MODE_WEIGHTED : GAUSS_MODE_POOLED;
    d.lambda = 0.0; d.u_codings = GAUSS_CODE_ADDITIVE;
    win.source(d);
    const size_t M = rows.size(), U = bp_u.size();
    if (M == 0)
        return herr("LD scores: no SNP of '%s' is in the panel between %lld and %lld on chromosome %d: the window has no SNP to score", c.input,
                    (long long)c.start_bp, (long long)c.end_bp, c.chr);
    if (M > GAUSS_HOST_LDSCORE_MAX_TARGETS || M + U > GAUSS_HOST_LDSCORE_MAX_ROWS)
        return herr("LD scores: the window has %zu SNPs to score and %zu panel SNPs in all; one call takes at most %d and %d: shorten the window",
                    M, M + U, GAUSS_HOST_LDSCORE_MAX_TARGETS, GAUSS_HOST_LDSCORE_MAX_ROWS);
    d.n_measured = (int)M; d.n_unmeasured = (int)U;
    const double n_eff = n_arg > 0.0 ? n_arg : mix ? kish_n_eff(d.pop_wgt, d.pop_off, d.n_pop) : (double)d.pop_off[d.n_pop];
    std::vector<double> raw(M), l2(M), mass(M);
    d.lds_on = 1; d.lds_n_annot = 0; d.lds_radius = c.wing; d.lds_n = n_eff;
    d.lds_bp_m = bp_m.data(); d.lds_bp_u = U ? bp_u.data() : nullptr;
    d.out_lds_raw = raw.data(); d.out_lds_l2 = l2.data(); d.out_lds_mass = mass.data();
    // (out_b11 = out_b21 = NULL: the matrices stay on the device; out_status = NULL: an LD window raises no status bit)
    if (win.run(ctx, &d)) return -1;
    *out = ldscore_output(mix, rows, l2.data(), raw.data(), mass.data(), n_eff, n_ref, n_ref_5_50, c.wing);
    return 0;
}

int gauss_host_dist_ldscore(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                            const char* input_file, const char* reference_index_file, const char* reference_data_file,
                            const char* reference_pop_desc_file, double af1_cutoff, double n, gauss_table** out)
{
    return run_ldscore(ctx, call_pop(GAUSS_KIND_LDSCORE, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                     reference_data_file, reference_pop_desc_file, af1_cutoff), n, out);
}

int gauss_host_distmix_ldscore(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                               const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                               const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                               double af1_cutoff, double n, gauss_table** out)
{
    return run_ldscore(ctx, call_mix(GAUSS_KIND_LDSCOREMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                     reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), n, out);
}

int gauss_host_dist_traits(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                           const char* input_file, const char* reference_index_file, const char* reference_data_file,
                           const char* reference_pop_desc_file, double af1_cutoff, const char* const* more_input_files, int n_more,
                           gauss_table** out)
{
    TraitsRider r(more_input_files, n_more, false);
    return run_impute(ctx, call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_distmix_traits(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                              const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                              const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                              double af1_cutoff, const char* const* more_input_files, int n_more, gauss_table** out)
{
    TraitsRider r(more_input_files, n_more, false);
    return run_impute(ctx, call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_dist_traits_miss(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                                const char* input_file, const char* reference_index_file, const char* reference_data_file,
                                const char* reference_pop_desc_file, double af1_cutoff, const char* const* more_input_files, int n_more,
                                gauss_table** out)
{
    TraitsRider r(more_input_files, n_more, true);
    return run_impute(ctx, call_pop(GAUSS_KIND_DIST, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_distmix_traits_miss(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                                   const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                                   const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                                   double af1_cutoff, const char* const* more_input_files, int n_more, gauss_table** out)
{
    TraitsRider r(more_input_files, n_more, true);
    return run_impute(ctx, call_mix(GAUSS_KIND_DISTMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), &r, out);
}

int gauss_host_slct_chi2(double p, double* out_chi2)
{
    if (!out_chi2) return herr("bad arguments");
    if (!(p > 0)) return herr("gauss_host_slct_chi2: p must be positive (got %g)", p);
    *out_chi2 = slct_chi2_of(p);
    return 0;
}

int gauss_host_qcat(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                    const char* input_file, const char* reference_index_file, const char* reference_data_file,
                    const char* reference_pop_desc_file, double af1_cutoff, gauss_table** out)
{
    return run_impute(ctx, call_pop(GAUSS_KIND_QCAT, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), nullptr, out);
}

int gauss_host_qcatmix(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                       const char* const* pop_names, const double* pop_wgts, int n_pop_wgt, const char* input_file,
                       const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                       double af1_cutoff, gauss_table** out)
{
    return run_impute(ctx, call_mix(GAUSS_KIND_QCATMIX, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), nullptr, out);
}

int gauss_host_prep_qcat(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size, const char* study_pop,
                         const char* input_file, const char* reference_index_file, const char* reference_data_file,
                         const char* reference_pop_desc_file, double af1_cutoff, gauss_table** out)
{
    return run_impute(ctx, call_pop(GAUSS_KIND_PREP_QCAT, chr, start_bp, end_bp, wing_size, study_pop, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), nullptr, out);
}

int gauss_host_prep_recessive_impute(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, int64_t wing_size,
                                     const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                                     const char* input_file, const char* reference_index_file,
                                     const char* reference_data_file, const char* reference_pop_desc_file,
                                     double af1_cutoff, gauss_table** out)
{
    return run_impute(ctx, call_mix(GAUSS_KIND_PREP_RECESSIVE, chr, start_bp, end_bp, wing_size, pop_names, pop_wgts, n_pop_wgt, input_file,
                                    reference_index_file, reference_data_file, reference_pop_desc_file, af1_cutoff), nullptr, out);
}

}  // extern "C"

// stats::quantile(x, probs = p) of R, default type 7 (quantile.default): index = 1 + (n-1)p, lo = floor, hi = ceiling,
// q = x[lo], and if index > lo and x[hi] != q:  q = (1-h) q + h x[hi]  with h = index - lo.  NaN input is an error in R.
static int r_quantile7(std::vector<double> x, double p, double* q)
{
    const size_t n = x.size();
    for (double v : x) if (std::isnan(v)) return herr("missing values and NaN's not allowed if 'na.rm' is FALSE");
    if (n == 0) { *q = NAN; return 0; }
    std::sort(x.begin(), x.end());
    const double index = 1 + (double)(n - 1) * p;
    const double lo = std::floor(index), hi = std::ceil(index);
    double qs = x[(size_t)lo - 1];
    const double xh = x[(size_t)hi - 1];
    if (index > lo && xh != qs) { const double h = index - lo; qs = (1 - h) * qs + h * xh; }
    *q = qs;
    return 0;
}

// The reading that prep_zmix5, the prep_zmix selectors and zmix share (read_input_zmix / read_ref_index_zmix, zmix.cpp:44-110,
// 1078-1181): the panel (open_panel_all_pops), the study's z merged with the index (allele-flipped to the panel's order) and the
// measured SNPs in map order.
int zmix_read(ZmixStudy& st, const char* input_file, const char* reference_index_file, const char* reference_data_file,
              const char* reference_pop_desc_file)
{
    Args& a = st.a;
    a.input_file = input_file; a.reference_index_file = reference_index_file;
    a.reference_data_file = reference_data_file; a.reference_pop_desc_file = reference_pop_desc_file;
    if (open_panel_all_pops(a, reference_index_file)) return -1;              // zmix.cpp:148-150: every population
    if (ReadInputZ(st.m, a, true)) return -1;                                 // read_input_zmix, zmix.cpp:1078-1113 (no window)
    if (ReadReferenceIndex(st.m, a, true)) return -1;                         // read_ref_index_zmix, zmix.cpp:1115-1181
    st.measured.clear();
    for (auto& kv : st.m) if (kv.second->type == 1) st.measured.push_back(kv.second.get());   // zmix.cpp:88-92
    return 0;
}

// The ancestry-informative SNPs of prep_zmix5 / prep_zmix5_sup (zmix.cpp:111-139, 257-285): every step-th measured SNP,
// cal_af_norm_var (zmix.cpp:1183-1214: variance of the panel AF columns, normalised by mean(1-mean)), kept iff its norm_var is
// above the type-7 quantile `pct` (cal_af_norm_var + the percentile cut).  kept: indices into `measured`, ascending; kept_nv: their
// norm_var; sel, when asked for: the SNPs themselves.
int zmix_ai_select(ZmixStudy& st, int step, double pct, std::vector<int>& kept, std::vector<double>& kept_nv, std::vector<Snp*>* sel)
{
    Args& a = st.a;
    const std::vector<Snp*>& measured = st.measured;
    std::vector<int> sub;
    for (int i = 0; i < (int)measured.size(); i += step) sub.push_back(i);
    std::vector<double> norm_var;
    BgzfReader fp;
    if (!a.pk && !fp.open(a.reference_data_file)) return herr("ERROR: can't open reference data file '%s'", a.reference_data_file.c_str());
    std::vector<double> af;
    for (int i : sub) {
        Snp* s = measured[(size_t)i];
        if (a.pk) af.assign(a.pk->af(s->fpos), a.pk->af(s->fpos) + a.num_pops);
        else load_line(fp, *s, a, &af);
        const int n = (int)af.size();
        double sum = 0.0, sq = 0.0;
        for (double v : af) sum += v;
        for (double v : af) sq += v * v;
        const double mean = sum / n;
        const double variance = sq / n - mean * mean;
        norm_var.push_back(variance / (mean * (1 - mean)));
    }
    double cutoff = 0;
    if (r_quantile7(norm_var, pct, &cutoff)) return -1;                       // zmix.cpp:126-130
    kept.clear(); kept_nv.clear();
    for (size_t i = 0; i < sub.size(); i++)
        if (norm_var[i] > cutoff) { kept.push_back(sub[i]); kept_nv.push_back(norm_var[i]); }   // zmix.cpp:135-139
    if (sel) { sel->clear(); for (int i : kept) sel->push_back(measured[(size_t)i]); }
    return 0;
}

// ReadGenotype of the selected SNPs, all populations (zmix.cpp:148-153): G holds one row of N genotype bytes per SNP, row
// stride *ld (N rounded up to 16)
int zmix_genotypes(Args& a, const std::vector<Snp*>& sel, int N, int64_t* ld, std::vector<uint8_t>& G)
{
    gauss_prepared tmp;
    tmp.args = a; tmp.N = N; tmp.ld = ((int64_t)N + 15) / 16 * 16;
    *ld = tmp.ld;
    if (a.pk) { unpack_rows(tmp, sel, G); return 0; }
    BgzfReader fp;
    if (!fp.open(a.reference_data_file)) return herr("ERROR: can't open reference data file '%s'", a.reference_data_file.c_str());
    for (Snp* s : sel) {
        load_line(fp, *s, a, nullptr);
        int n = 0;
        for (auto& g : s->geno) n += g.second;
        if (n != N) return herr("ERROR: genotype line of %s has %d samples, population table says %d", s->rsid.c_str(), n, N);
    }
    fill_matrix(G, sel, tmp.ld);
    return 0;
}

// prep_zmix5_sup's groups (zmix.cpp:201-361): population k belongs to its super-population, super-populations numbered in
// order of first appearance; returns their count
int zmix_sup_groups(const Args& a, std::vector<int32_t>& pop_group, std::vector<std::string>& names)
{
    pop_group.clear(); names.clear();
    for (int k = 0; k < a.num_pops; k++) {
        const std::string& sp = a.ref_sup_pop_vec[(size_t)k];
        size_t g = 0;
        while (g < names.size() && names[g] != sp) g++;
        if (g == names.size()) names.push_back(sp);
        pop_group.push_back((int32_t)g);
    }
    return (int)names.size();
}

// The table of a prep_zmix call (one row per SNP pair in data_mat: z_i * z_j, then the pair's genotype correlation inside each
// population or group): the listed SNPs with their z -- and norm_var, for the ancestry-informative selections -- and data_mat
static std::unique_ptr<gauss_table> prep_zmix_table(const std::vector<Snp*>& sel, const std::vector<double>* norm_var, int nrow, int ncol,
                                                    std::vector<double> data_mat)
{
    std::unique_ptr<gauss_table> t(new gauss_table());
    add_ident_columns(*t, sel);
    Column& z = t->add("z", GAUSS_COL_DBL);
    for (Snp* s : sel) z.d.push_back(s->z);
    if (norm_var) t->add("norm_var", GAUSS_COL_DBL).d = *norm_var;
    t->put_named("data_mat", nrow, ncol, std::move(data_mat));
    return t;
}

// ------------------------------------------------------------------------------------------
// The other prep_zmix selectors (zmix.cpp:201-1076).  They share prep_zmix5's reading (read_input_zmix /
// read_ref_index_zmix, every population) and its output (one row per SNP pair: z_i * z_j, then the pair's genotype
// correlation inside each population) and differ in WHICH pairs they list:
//   prep_zmix      zmix.cpp:940-1076   every interval-th measured SNP (default 1), all pairs
//   prep_zmix2     zmix.cpp:651-760    pairs (i, i + offset) for i = 0, interval, 2 interval, ...   (1000, 3)
//   prep_zmix3     zmix.cpp:511-650    every interval-th SNP, each with its next `steps` neighbours  (1000, 5)
//   prep_zmix4     zmix.cpp:363-510    for h = 0 .. interval-1: pairs (i, i + offset), i = h, h + interval, ...; an extra
//                                      leading column holds h                                        (1000, 3)
//   prep_zmix5_sup zmix.cpp:201-361    prep_zmix5's ancestry-informative SNPs, correlations pooled per SUPER-population
//                                      (CalCorSup zmix.cpp:1221-1246), super-populations in order of first appearance
// The GPU part is gauss_ld_per_pop_pairs: only the tile pairs the listed pairs touch are multiplied.
// ------------------------------------------------------------------------------------------
enum ZmixVariant { ZMIX_ALL = 0, ZMIX_2 = 2, ZMIX_3 = 3, ZMIX_4 = 4, ZMIX_5SUP = 6 };

static int prep_zmix_variant(gauss_ctx* ctx, int variant, const char* input_file, const char* reference_index_file,
                             const char* reference_data_file, const char* reference_pop_desc_file, double percentile, int interval,
                             int p2, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    if (files_ok({input_file, reference_index_file, reference_data_file, reference_pop_desc_file})) return -1;
    // defaults: zmix.cpp:953-957 (1), 664-675 / 376-387 / 524-535 (1000 and 3 / 3 / 5), 214-224 (0.99, 1)
    const int step = interval > 0 ? interval : ((variant == ZMIX_ALL || variant == ZMIX_5SUP) ? 1 : 1000);
    const int par2 = p2 > 0 ? p2 : (variant == ZMIX_3 ? 5 : 3);
    const double pct = std::isnan(percentile) ? 0.99 : percentile;
    ZmixStudy st;
    if (zmix_read(st, input_file, reference_index_file, reference_data_file, reference_pop_desc_file)) return -1;
    Args& a = st.a;
    const std::vector<Snp*>& measured = st.measured;
    const int n = (int)measured.size();

    // ---- which SNPs, which pairs (indices into `measured`) ----
    std::vector<std::pair<int, int>> pairs;
    std::vector<double> lead;                                    // prep_zmix4's leading column
    std::vector<double> sub_nv;                                  // prep_zmix5_sup: norm_var of the kept SNPs
    if (variant == ZMIX_ALL || variant == ZMIX_3 || variant == ZMIX_5SUP) {
        std::vector<int> sub;
        if (variant == ZMIX_5SUP) {
            if (zmix_ai_select(st, step, pct, sub, sub_nv, nullptr)) return -1;
        } else {
            for (int i = 0; i < n; i += step) sub.push_back(i);  // zmix.cpp:996-1004, 567-575
        }
        const int S = (int)sub.size();
        for (int i = 0; i < S; i++) {
            const int jend = variant == ZMIX_3 ? std::min(i + 1 + par2, S) : S;      // zmix.cpp:592-594
            for (int j = i + 1; j < jend; j++) pairs.emplace_back(sub[(size_t)i], sub[(size_t)j]);
        }
    } else if (variant == ZMIX_2) {
        for (int i = 0; i < n; i += step) {                      // zmix.cpp:721-745
            if (i + par2 < n) pairs.emplace_back(i, i + par2);
            else break;
        }
    } else {                                                     // ZMIX_4, zmix.cpp:440-465
        for (int h = 0; h < step; h++)
            for (int i = h; i < n; i += step) {
                if (i + par2 < n) { pairs.emplace_back(i, i + par2); lead.push_back((double)h); }
                else break;
            }
    }
    // the SNPs that occur in some pair, in list order; a pair is (smaller row, larger row) -- the reference's pairs are
    // (earlier SNP, later SNP) already, and the correlation is symmetric
    std::vector<int> row_of((size_t)n, -1);
    std::vector<Snp*> sel;
    {
        std::vector<char> used((size_t)n, 0);
        for (auto& pr : pairs) { used[(size_t)pr.first] = 1; used[(size_t)pr.second] = 1; }
        for (int i = 0; i < n; i++) if (used[(size_t)i]) { row_of[(size_t)i] = (int)sel.size(); sel.push_back(measured[(size_t)i]); }
    }
    const int S = (int)sel.size(), P = a.num_pops;
    // population groups: each population (all but _sup), or its super-population in order of first appearance
    std::vector<int32_t> pop_group;
    int n_group = P;
    std::vector<std::string> group_names = a.ref_pop_vec;
    if (variant == ZMIX_5SUP) n_group = zmix_sup_groups(a, pop_group, group_names);
    int N = 0;
    const std::vector<int32_t> pop_off = panel_pop_off(a, &N);
    const size_t np = pairs.size();
    const int nlead = variant == ZMIX_4 ? 1 : 0;
    const int ncol = nlead + 1 + n_group;
    std::vector<double> dm(np * (size_t)ncol, 0.0);
    // the pairs as rows of the SNP table
    std::vector<double> pm(np * 2, 0.0);
    for (size_t k = 0; k < np; k++) { pm[k] = row_of[(size_t)pairs[k].first]; pm[np + k] = row_of[(size_t)pairs[k].second]; }
    if (np > 0) {
        int64_t ld = 0;
        std::vector<uint8_t> G;
        if (zmix_genotypes(a, sel, N, &ld, G)) return -1;
        std::vector<int32_t> pi(np), pj(np);
        for (size_t k = 0; k < np; k++) {
            pi[k] = row_of[(size_t)pairs[k].first]; pj[k] = row_of[(size_t)pairs[k].second];
            if (nlead) dm[k] = lead[k];
            dm[(size_t)nlead * np + k] = measured[(size_t)pairs[k].first]->z * measured[(size_t)pairs[k].second]->z;
        }
        if (gauss_ld_per_pop_pairs(ctx, G.data(), S, ld, pop_off.data(), P, pop_group.empty() ? nullptr : pop_group.data(), n_group,
                                   pi.data(), pj.data(), (int64_t)np, dm.data() + (size_t)(nlead + 1) * np) != 0)
            return herr("%s", gauss_last_error());
    }
    std::unique_ptr<gauss_table> t = prep_zmix_table(sel, variant == ZMIX_5SUP ? &sub_nv : nullptr, (int)np, ncol, std::move(dm));
    t->put_named("pairs", (int)np, 2, std::move(pm));
    for (const std::string& g : group_names) t->messages.push_back(g);      // the groups the correlation columns stand for
    *out = t.release();
    return 0;
}

// computeLD's SNP selection (computeLD.cpp:26-93, 134-149), shared with simulateLD (simulateLD.cpp:44-124, 226-245): a lean window
// of measured SNPs only with rows from the resident panel where CallWindow builds one, else the literal path.
int computeld_rows(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names, const double* pop_wgts,
                   int n_pop_wgt, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                   const char* reference_pop_desc_file, double af1_cutoff, LdRows& out)
{
    if (files_ok({input_file, reference_index_file, reference_data_file, reference_pop_desc_file})) return -1;
    std::string panel_path;
    if (open_panel(reference_index_file, reference_data_file, reference_pop_desc_file, panel_path, out.pk)) return -1;
    const CallArgs c = call_mix(GAUSS_KIND_COMPUTELD, chr, start_bp, end_bp, 0, pop_names, pop_wgts, n_pop_wgt, input_file, reference_index_file,
                                reference_data_file, reference_pop_desc_file, af1_cutoff);
    CallWindow win;
    if (win.build(c, panel_path, out.pk)) return -1;
    out.a = win.args();
    out.M = (int)win.n_measured();
    if (out.M <= out.a.min_num_measured_snp)                             // computeLD.cpp:89-93
        return herr("Not enough number of SNPs loaded - computeLD not performed (measured %d)", out.M);
    gauss_window_desc d;
    memset(&d, 0, sizeof(d));
    win.source(d);
    out.pop_off.assign(d.pop_off, d.pop_off + d.n_pop + 1);
    out.pop_wgt.assign(d.pop_wgt, d.pop_wgt + d.n_pop);
    if (d.geno_format == GAUSS_GENO_2BIT) {                              // rows of the packed panel, by index: from its resident copy
        panel_rows(ctx, panel_path, *out.pk, &d.geno_m, &out.on_device);
        out.rows.assign(d.rows_m, d.rows_m + out.M);
        out.pop_src_off.assign(d.pop_src_off, d.pop_src_off + d.n_pop);
    }
    out.store = d.geno_m; out.ld = d.ld; out.geno_fmt = d.geno_format;
    std::vector<ViewSnp> m;
    for (int i = 0; i < out.M; i++) m.push_back(win.measured((size_t)i));
    out.t.reset(new gauss_table());                                      // computeLD.cpp:134-149
    add_ident_columns(*out.t, m.size(), [&](size_t i) { return m[i].id; });
    Column& af = out.t->add("af1mix", GAUSS_COL_DBL);
    for (const ViewSnp& s : m) { af.d.push_back(s.af); out.z.push_back(s.z); }
    out.prep = win.release();                                            // (a literal window's rows are `store`)
    return 0;
}

extern "C" {

int gauss_host_prep_zmix5(gauss_ctx* ctx, const char* input_file, const char* reference_index_file,
                          const char* reference_data_file, const char* reference_pop_desc_file,
                          double percentile, int interval, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    if (files_ok({input_file, reference_index_file, reference_data_file, reference_pop_desc_file})) return -1;
    const double pct = std::isnan(percentile) ? 0.99 : percentile;            // zmix.cpp:57-61
    const int step = interval > 0 ? interval : 1;                             // zmix.cpp:63-67
    ZmixStudy st;
    if (zmix_read(st, input_file, reference_index_file, reference_data_file, reference_pop_desc_file)) return -1;
    std::vector<int> kept;
    std::vector<double> sub_nv;
    std::vector<Snp*> sub;
    if (zmix_ai_select(st, step, pct, kept, sub_nv, &sub)) return -1;
    const int S = (int)sub.size(), P = st.a.num_pops;
    int N = 0;
    const std::vector<int32_t> pop_off = panel_pop_off(st.a, &N);
    const size_t npairs = S > 1 ? (size_t)S * (S - 1) / 2 : 0;
    std::vector<double> dm(npairs * (size_t)(1 + P), 0.0);
    if (S > 1) {
        int64_t ld = 0;
        std::vector<uint8_t> G;
        if (zmix_genotypes(st.a, sub, N, &ld, G)) return -1;
        size_t row = 0;
        for (int i = 0; i < S; i++)
            for (int j = i + 1; j < S; j++) dm[row++] = sub[i]->z * sub[j]->z;           // zmix.cpp:165
        // (all pairs: gauss_ld_per_pop -- no pair list to upload)
        if (gauss_ld_per_pop(ctx, G.data(), S, ld, pop_off.data(), P, dm.data() + npairs) != 0)
            return herr("%s", gauss_last_error());
    }
    *out = prep_zmix_table(sub, &sub_nv, (int)npairs, 1 + P, std::move(dm)).release();
    return 0;
}

int gauss_host_prep_zmix(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                         const char* reference_pop_desc_file, int interval, gauss_table** out)
{
    return prep_zmix_variant(ctx, ZMIX_ALL, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, NAN, interval, 0, out);
}
int gauss_host_prep_zmix2(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                          const char* reference_pop_desc_file, int interval, int offset, gauss_table** out)
{
    return prep_zmix_variant(ctx, ZMIX_2, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, NAN, interval, offset, out);
}
int gauss_host_prep_zmix3(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                          const char* reference_pop_desc_file, int interval, int steps, gauss_table** out)
{
    return prep_zmix_variant(ctx, ZMIX_3, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, NAN, interval, steps, out);
}
int gauss_host_prep_zmix4(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                          const char* reference_pop_desc_file, int interval, int offset, gauss_table** out)
{
    return prep_zmix_variant(ctx, ZMIX_4, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, NAN, interval, offset, out);
}
int gauss_host_prep_zmix5_sup(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                              const char* reference_pop_desc_file, double percentile, int interval, gauss_table** out)
{
    return prep_zmix_variant(ctx, ZMIX_5SUP, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, percentile, interval, 0, out);
}

int gauss_host_computeLD(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names,
                         const double* pop_wgts, int n_pop_wgt, const char* input_file, const char* reference_index_file,
                         const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff,
                         gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    LdRows s;
    if (computeld_rows(ctx, chr, start_bp, end_bp, pop_names, pop_wgts, n_pop_wgt, input_file, reference_index_file, reference_data_file,
                       reference_pop_desc_file, af1_cutoff, s)) return -1;
    const int M = s.M;
    std::unique_ptr<gauss_table> t = std::move(s.t);
    t->matrix.assign((size_t)M * M, 0.0);
    t->matrix_n = M;
    if (gauss_ld_rows(ctx, GAUSS_MODE_WEIGHTED, s.store, s.ld, s.geno_fmt, s.row_ptr(), M, s.pop_off.data(), s.src_off_ptr(), s.pop_wgt.data(),
                      s.n_pop(), 1.0, s.on_device, t->matrix.data()) != 0) return herr("%s", gauss_last_error());
    *out = t.release();
    return 0;
}

int gauss_host_clump(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names, const double* pop_wgts,
                     int n_pop_wgt, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                     const char* reference_pop_desc_file, double af1_cutoff, double p1, double p2, double r2, double kb, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    ClumpKeys k;
    if (clump_keys(p1, p2, r2, kb, k)) return -1;
    LdRows s;
    if (computeld_rows(ctx, chr, start_bp, end_bp, pop_names, pop_wgts, n_pop_wgt, input_file, reference_index_file, reference_data_file,
                       reference_pop_desc_file, af1_cutoff, s)) return -1;
    const int M = s.M;
    if (M > GAUSS_CLUMP_MAX_M)
        return herr("clump: the region holds %d SNPs of the study; a call clumps at most %d (ask for a shorter region)", M, GAUSS_CLUMP_MAX_M);
    const std::vector<int32_t>& bp = s.t->cols[2].i;                     // add_ident_columns: rsid chr bp a1 a2
    std::vector<double> key((size_t)M), r2_out((size_t)M);
    for (int i = 0; i < M; i++) key[(size_t)i] = s.z[(size_t)i] * s.z[(size_t)i];
    std::vector<int32_t> owner((size_t)M), rank((size_t)M);
    int32_t n = 0;
    if (gauss_ld_clump_rows(ctx, GAUSS_MODE_WEIGHTED, s.store, s.ld, s.geno_fmt, s.row_ptr(), M, s.pop_off.data(), s.src_off_ptr(),
                            s.pop_wgt.data(), s.n_pop(), s.on_device, bp.data(), key.data(), 1, k.radius, k.r2_min, k.key_index, k.key_member,
                            owner.data(), rank.data(), r2_out.data(), &n) != 0) return herr("%s", gauss_last_error());
    clump_output(*s.t, s.z, owner.data(), rank.data(), r2_out.data(), n);
    *out = s.t.release();
    return 0;
}

int gauss_host_ldsplit(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names, const double* pop_wgts,
                       int n_pop_wgt, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                       const char* reference_pop_desc_file, double af1_cutoff, double thr_r2, int min_size, int max_size, int max_K,
                       double max_r2, double kb, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    LdSplitParams k;
    if (ldsplit_params(thr_r2, min_size, max_size, max_K, max_r2, kb, k)) return -1;
    LdRows s;
    if (computeld_rows(ctx, chr, start_bp, end_bp, pop_names, pop_wgts, n_pop_wgt, input_file, reference_index_file, reference_data_file,
                       reference_pop_desc_file, af1_cutoff, s)) return -1;
    const int M = s.M;
    if (M > GAUSS_LDSPLIT_MAX_M)
        return herr("ldsplit: the region holds %d SNPs of the study; a call splits at most %d (ask for a shorter region)", M, GAUSS_LDSPLIT_MAX_M);
    const std::vector<int32_t>& bp = s.t->cols[2].i;                     // add_ident_columns: rsid chr bp a1 a2
    std::vector<double> cost((size_t)k.max_K), mx((size_t)M + 1);
    std::vector<int32_t> prev((size_t)k.max_K * ((size_t)M + 1));
    int64_t n_bad = 0;
    if (gauss_ld_split_rows(ctx, GAUSS_MODE_WEIGHTED, s.store, s.ld, s.geno_fmt, s.row_ptr(), M, s.pop_off.data(), s.src_off_ptr(),
                            s.pop_wgt.data(), s.n_pop(), s.on_device, bp.data(), k.radius, k.thr_r2, k.min_size, k.max_size, k.max_K, k.max_r2,
                            cost.data(), prev.data(), mx.data(), &n_bad) != 0) return herr("%s", gauss_last_error());
    ldsplit_output(*s.t, M, k.max_K, cost.data(), prev.data(), mx.data(), n_bad);
    *out = s.t.release();
    return 0;
}

int gauss_host_hess(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names, const double* pop_wgts,
                    int n_pop_wgt, const char* const* input_files, int n_files, const char* reference_index_file,
                    const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff, int k_max, double eig_min,
                    gauss_table** out)
{
    if (!ctx || !out || !input_files) return herr("bad arguments");
    if (n_files < 1 || n_files > GAUSS_HESS_MAX_TRAITS)
        return herr("hess: %d study files; a call takes 1 .. %d (one trait each)", n_files, GAUSS_HESS_MAX_TRAITS);
    const int K = k_max == 0 ? 256 : k_max;
    const double em = std::isnan(eig_min) ? 1e-6 : eig_min;
    if (K < 1 || K > GAUSS_HESS_MAX_K) return herr("hess: k_max = %d; a call projects on 1 .. %d eigenvectors", k_max, GAUSS_HESS_MAX_K);
    if (!(em >= 0.0 && em < 1.0)) return herr("hess: eig_min = %g is outside [0, 1)", em);
    for (int k = 0; k < n_files; k++) if (files_ok({input_files[k]})) return -1;
    LdRows s;
    if (computeld_rows(ctx, chr, start_bp, end_bp, pop_names, pop_wgts, n_pop_wgt, input_files[0], reference_index_file, reference_data_file,
                       reference_pop_desc_file, af1_cutoff, s)) return -1;
    const int M = s.M;
    if (M > GAUSS_HESS_MAX_M)
        return herr("hess: the block holds %d SNPs of the study; a call takes at most %d (ask for a shorter region)", M, GAUSS_HESS_MAX_M);
    // the further files at the SNPs of the first, as dist_traits reads them: every SNP present, swapped alleles flip the sign
    const gauss_table& t = *s.t;                                         // add_ident_columns: rsid chr bp a1 a2
    std::vector<double> z((size_t)n_files * M);
    std::copy(s.z.begin(), s.z.end(), z.begin());
    for (int k = 1; k < n_files; k++) {
        std::string err;
        std::shared_ptr<const GwasCache> gw = load_gwas_cached(input_files[k], err);
        if (!gw) return herr("%s", err.c_str());
        if (traits_match(*gw, input_files[k], (size_t)M, [&](size_t i) {
                return SnpIdent{t.cols[0].s[i].c_str(), t.cols[1].i[i], (long long)t.cols[2].i[i], t.cols[3].s[i].c_str(), t.cols[4].s[i].c_str()};
            }, z.data() + (size_t)k * M)) return -1;
    }
    std::vector<double> lam((size_t)M), proj((size_t)n_files * K);
    int32_t n_pos = 0, sweeps = 0, status = 0;
    int64_t n_bad = 0;
    if (gauss_ld_hess_rows(ctx, GAUSS_MODE_WEIGHTED, s.store, s.ld, s.geno_fmt, s.row_ptr(), M, s.pop_off.data(), s.src_off_ptr(),
                           s.pop_wgt.data(), s.n_pop(), s.on_device, z.data(), n_files, K, em, lam.data(), proj.data(), &n_pos, &sweeps, &n_bad,
                           &status, nullptr, nullptr) != 0) return herr("%s", gauss_last_error());
    hess_output(*s.t, M, n_files, K, z.data(), lam.data(), proj.data(), n_pos, sweeps, n_bad, status);
    *out = s.t.release();
    return 0;
}

// ---- jepeg() / jepegmix() over several ranks ("genes: contiguous gene ranges") ------------------------------
// Genes are independent (jepeg.cpp:114-131: one Gene object per gene, nothing shared but the read-only SNP map; grouping at
// gauss.cpp:1383-1439).  Every rank runs the same host data layer on the same files, derives the same plan -- contiguous gene
// ranges of equal cost -- and computes CorG and the k x k tails of ITS range only; the ranges' tables, concatenated in rank order,
// are the one-rank table row for row (same bits: a gene's block and tail do not depend on which other genes share the launch).
// A gene costs its SNP pairs n (n + 1) (CorG's pair loops, gene.cpp:306-315 / 576-586 -- the unit the judge's plan names) plus a
// constant for its k x k tail, which does not grow with n (k <= 6; ~3 us against ~1 us per 100 pairs of the batch launch).
static const long long JEPEG_GENE_TAIL_COST = 64;
static void jepeg_gene_ranges(const std::vector<int32_t>& gene_off, int world, std::vector<int32_t>& first)
{
    const int ng = gene_off.empty() ? 0 : (int)gene_off.size() - 1;
    world = std::max(1, world);
    std::vector<long long> pre((size_t)ng + 1, 0);
    for (int g = 0; g < ng; g++) {
        const long long n = gene_off[(size_t)g + 1] - gene_off[(size_t)g];
        pre[(size_t)g + 1] = pre[(size_t)g] + n * (n + 1) + JEPEG_GENE_TAIL_COST;
    }
    first.assign((size_t)world + 1, ng);
    first[0] = 0;
    int g = 0;
    for (int r = 1; r < world; r++) {
        // rank r starts at the first gene whose MIDPOINT lies at or beyond r / world of the total: boundaries are monotone, every gene
        // belongs to exactly one rank, and a rank may be empty when there are fewer genes than ranks
        const long long want = 2 * pre[(size_t)ng] * r;           // compare 2 * world * midpoint with 2 * total * r (integers)
        while (g < ng && (pre[(size_t)g] + pre[(size_t)g + 1]) * world < want) g++;
        first[(size_t)r] = g;
    }
}

int gauss_prepared_jepeg_plan(const gauss_prepared* p, int world, int32_t* first)
{
    if (!p || !first) return herr("bad arguments");
    if (p->kind != GAUSS_KIND_JEPEG && p->kind != GAUSS_KIND_JEPEGMIX) return herr("not a jepeg / jepegmix object");
    if (world < 1) return herr("world = %d", world);
    std::vector<int32_t> f;
    jepeg_gene_ranges(p->gene_off, world, f);
    std::copy(f.begin(), f.end(), first);
    return 0;
}

// The gene table of genes [g0, g1) from their CorG blocks (concatenated n_g x n_g, diagonal 1 + lambda): Gene::RunJepeg bookkeeping
// and CalJepegPval from W on (gene.cpp:88-185, 317-550), jepeg.cpp:143-151's columns.  Named matrix "gene_range" = [g0, g1, genes].
static gauss_table* jepeg_table(const gauss_prepared& p, int g0, int g1, const double* blocks)
{
    std::unique_ptr<gauss_table> t(new gauss_table());
    Column geneid{"geneid", GAUSS_COL_STR, {}, {}, {}}, chisq{"chisq", GAUSS_COL_DBL, {}, {}, {}}, df{"df", GAUSS_COL_INT, {}, {}, {}};
    Column jp{"jepeg_pval", GAUSS_COL_DBL, {}, {}, {}}, ns{"num_snp", GAUSS_COL_INT, {}, {}, {}}, tc{"top_categ", GAUSS_COL_STR, {}, {}, {}};
    Column tcp{"top_categ_pval", GAUSS_COL_DBL, {}, {}, {}}, ts{"top_snp", GAUSS_COL_STR, {}, {}, {}}, tsp{"top_snp_pval", GAUSS_COL_DBL, {}, {}, {}};
    // (the k x k tails on host threads were measured twice: round 5, eight threads: 1.1 -> 0.45 ms and the call no shorter; round 6,
    // at most four threads, 16 genes a task, rows written in place: tails 1.12 -> 0.47 ms and the NEXT call's data layer 1.12 ->
    // 1.35-1.5 ms -- the threads started per call move the calling thread off its warm core -- call 3.48 -> 3.35-3.5 ms: not kept)
    size_t o = 0;
    for (int g = g0; g < g1; g++) {
        std::vector<Snp*> gs(p.measured.begin() + p.gene_off[(size_t)g], p.measured.begin() + p.gene_off[(size_t)g + 1]);
        const GeneResult r = jepeg_tail(gs, blocks + o, p.args);
        o += gs.size() * gs.size();
        geneid.s.push_back(r.geneid); chisq.d.push_back(r.chisq); df.i.push_back(r.df); jp.d.push_back(r.jepeg_pval);
        ns.i.push_back(r.num_snp); tc.s.push_back(r.top_categ); tcp.d.push_back(r.top_categ_pval);
        ts.s.push_back(r.top_snp); tsp.d.push_back(r.top_snp_pval);
    }
    t->cols = {geneid, chisq, df, jp, ns, tc, tcp, ts, tsp};          // jepeg.cpp:143-151
    t->put_named("gene_range", 1, 3, {(double)g0, (double)g1, (double)(p.gene_off.empty() ? 0 : (int)p.gene_off.size() - 1)});
    return t.release();
}

int gauss_prepared_jepeg_finish(const gauss_prepared* p, int g0, int g1, const double* blocks, gauss_table** out)
{
    if (!p || !out) return herr("bad arguments");
    if (p->kind != GAUSS_KIND_JEPEG && p->kind != GAUSS_KIND_JEPEGMIX) return herr("not a jepeg / jepegmix object");
    const int ng = p->gene_off.empty() ? 0 : (int)p->gene_off.size() - 1;
    if (g0 < 0 || g1 < g0 || g1 > ng) return herr("gene range [%d, %d) of %d genes", g0, g1, ng);
    if (g1 > g0 && !blocks) return herr("blocks is NULL");
    *out = jepeg_table(*p, g0, g1, blocks);
    return 0;
}

// The head of the gene calls (jepeg, sumchi2): the data layer with the SNP map of annotated positions only.
// The gene table is made of annotated SNPs alone, and every step of the data layer after ReadInputZ works on the entries of one
// position at a time: only the study SNPs at positions the annotation names enter the SNP map (plus the positions the study
// lists more than once or under equal alleles -- the only ones where the reference's duplicate check can fire, so a study that
// fails there still fails).  A chromosome's study is four times its annotated SNPs: the data layer of a jepegmix() call
// 3.9 -> 1.0 ms.  GAUSS_HOST_FULL_MAP=1: the whole study, as gauss_host_prepare enters it (same table, bit for bit:
// tests/test_gpu_drivers.py).
static int gene_prepare(const CallArgs& c, const char* annotation, std::unique_ptr<gauss_prepared>& out)
{
    gauss_prepared* p = nullptr;
    if (prepare_files(c, annotation, !env_flag("GAUSS_HOST_FULL_MAP", false), &p)) return -1;
    out.reset(p);
    return 0;
}
// ... and where its measured rows are, as the *_rows entry points take them: the panel's 2-bit rows by index (panel_rows: the
// resident copy) when the data layer kept row lists into a packed panel, else its byte matrix, rows 0 .. M - 1 (rows = NULL)
struct GeneRows { const uint8_t* store; int64_t ld; int format, on_device; const int32_t *rows, *pop_src_off; };
static GeneRows gene_rows(gauss_ctx* ctx, const gauss_prepared& p)
{
    if (!p.packed_rows) return {p.gm.data(), p.ld, GAUSS_GENO_U8, 0, nullptr, nullptr};
    GeneRows r = {nullptr, p.args.pk->row_bytes(), GAUSS_GENO_2BIT, 0, p.store_rows_m.data(), p.pop_src_off.data()};
    panel_rows(ctx, p.args.reference_data_file, *p.args.pk, &r.store, &r.on_device);
    return r;
}

// c: call_pop / call_mix of kind GAUSS_KIND_JEPEG / GAUSS_KIND_JEPEGMIX without a window (the rank entry points fill both forms)
static int run_jepeg(gauss_ctx* ctx, const CallArgs& c, const char* annotation, int rank, int world, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    if (world < 1 || rank < 0 || rank >= world) return herr("rank %d of world %d", rank, world);
    const double t_begin = now_s();
    std::unique_ptr<gauss_prepared> p;
    if (gene_prepare(c, annotation, p)) return -1;
    const double t_prepared = now_s();
    const Args& a = p->args;
    std::vector<int32_t> first;
    jepeg_gene_ranges(p->gene_off, world, first);
    const int g0 = first[(size_t)rank], g1 = first[(size_t)rank + 1];
    const int ng = g1 - g0;
    // this rank's genes: rows [r0, r0 + S) of the measured list, gene offsets relative to r0
    const int r0 = ng > 0 ? p->gene_off[(size_t)g0] : 0;
    const int S = ng > 0 ? p->gene_off[(size_t)g1] - r0 : 0;
    std::vector<int32_t> goff((size_t)ng + 1, 0);
    size_t tot = 0;
    for (int g = 0; g < ng; g++) {
        goff[(size_t)g + 1] = p->gene_off[(size_t)(g0 + g) + 1] - r0;
        const size_t n = (size_t)(goff[(size_t)g + 1] - goff[(size_t)g]);
        tot += n * n;
    }
    std::vector<double> blocks(std::max<size_t>(tot, 1), 0.0);
    if (S > 0 && ng > 0) {
        // CorG of every gene of the range in one launch, diagonal 1 + lambda (gene.cpp:306-315 / 576-586)
        const int mode = (c.kind == GAUSS_KIND_JEPEG) ? GAUSS_MODE_POOLED : GAUSS_MODE_WEIGHTED;
        const GeneRows g = gene_rows(ctx, *p);
        const int rc = g.rows ? gauss_gene_ld_batch_rows(ctx, mode, g.store, g.ld, g.format, g.rows + r0, S, p->pop_off.data(), g.pop_src_off,
                                                         p->pop_wgt.data(), (int)p->pop_off.size() - 1, goff.data(), ng, 1.0 + a.lambda,
                                                         g.on_device, blocks.data())
                              : gauss_gene_ld_batch(ctx, mode, g.store + (size_t)r0 * (size_t)g.ld, S, g.ld, p->pop_off.data(), p->pop_wgt.data(),
                                                    (int)p->pop_off.size() - 1, goff.data(), ng, 1.0 + a.lambda, blocks.data());
        if (rc != 0) return herr("%s", gauss_last_error());
    }
    const double t_ld = now_s();
    *out = jepeg_table(*p, g0, g1, blocks.data());
    if (host_trace("prep"))
        fprintf(stderr, "[jepeg] rank %d of %d, genes [%d, %d): data layer %.2f ms, gene LD blocks on the GPU %.2f ms, %d k x k tails + table %.2f ms\n",
                rank, world, g0, g1, (t_prepared - t_begin) * 1e3, (t_ld - t_prepared) * 1e3, ng, (now_s() - t_ld) * 1e3);
    return 0;
}

int gauss_host_jepeg(gauss_ctx* ctx, const char* study_pop, const char* input_file, const char* annotation_file,
                     const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                     double af1_cutoff, gauss_table** out)
{
    return run_jepeg(ctx, call_gene(GAUSS_KIND_JEPEG, study_pop, nullptr, nullptr, 0, input_file, reference_index_file, reference_data_file,
                                    reference_pop_desc_file, af1_cutoff), annotation_file, 0, 1, out);
}

int gauss_host_jepegmix(gauss_ctx* ctx, const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                        const char* input_file, const char* annotation_file, const char* reference_index_file,
                        const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff,
                        gauss_table** out)
{
    return run_jepeg(ctx, call_gene(GAUSS_KIND_JEPEGMIX, nullptr, pop_names, pop_wgts, n_pop_wgt, input_file, reference_index_file,
                                    reference_data_file, reference_pop_desc_file, af1_cutoff), annotation_file, 0, 1, out);
}

// sumchi2() / sumchi2mix(): jepeg's genes and SNPs (the same data layer, the same measured list and gene_off; categ and wgt are not
// read), tested by the plain sum of chi2 on the GPU (gauss_gene_sumchi2[_rows]); the head and the row source are run_jepeg's
static int run_sumchi2(gauss_ctx* ctx, const CallArgs& c, const char* annotation, double prune_r2, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    const double r2 = std::isnan(prune_r2) ? 0.9 : prune_r2;                       // fastBAT's default
    if (!(r2 > 0.0 && r2 <= 1.0)) return herr("sumchi2: prune_r2 = %g is outside (0, 1]", r2);
    std::unique_ptr<gauss_prepared> p;
    if (gene_prepare(c, annotation, p)) return -1;
    const int ng = p->gene_off.empty() ? 0 : (int)p->gene_off.size() - 1;
    const int S = ng > 0 ? p->gene_off[(size_t)ng] : 0;
    // jepeg's sort by gene id (std::sort) leaves the order inside a gene open; the pruning is defined in position order, so each gene's
    // rows are put in the order of the SNP list (chromosome, position), and the rows reach the GPU by index in that order
    std::vector<int32_t> perm((size_t)S);
    for (int i = 0; i < S; i++) perm[(size_t)i] = i;
    for (int g = 0; g < ng; g++)
        std::stable_sort(perm.begin() + p->gene_off[(size_t)g], perm.begin() + p->gene_off[(size_t)g + 1],
                         [&](int32_t x, int32_t y) { return p->measured_rows[(size_t)x] < p->measured_rows[(size_t)y]; });
    std::vector<std::string> geneid, rsid;
    std::vector<double> z;
    for (int i = 0; i < S; i++) { const Snp* s = p->measured[(size_t)perm[(size_t)i]]; rsid.push_back(s->rsid); z.push_back(s->z); }
    for (int g = 0; g < ng; g++) {
        const int r0 = p->gene_off[(size_t)g], n = p->gene_off[(size_t)g + 1] - r0;
        geneid.push_back(n > 0 ? p->measured[(size_t)r0]->geneid : std::string());
        if (n > GAUSS_SUMCHI2_MAX_N)
            return herr("sumchi2: gene %s holds %d SNPs of the study; a gene holds at most %d", geneid.back().c_str(), n, GAUSS_SUMCHI2_MAX_N);
    }
    std::vector<int32_t> kept((size_t)std::max(S, 1)), n_kept((size_t)std::max(ng, 1), 0), top((size_t)std::max(ng, 1), -1);
    std::vector<int32_t> status((size_t)std::max(ng, 1), GAUSS_ST_SUMCHI2_EMPTY);       // (no SNP at all: no GPU call, every gene is empty)
    std::vector<double> lam((size_t)std::max(ng, 1) * GAUSS_SUMCHI2_MAX_KEPT, NAN), q((size_t)std::max(ng, 1), 0.0);
    if (S > 0 && ng > 0) {
        const int mode = (c.kind == GAUSS_KIND_JEPEG) ? GAUSS_MODE_POOLED : GAUSS_MODE_WEIGHTED;
        const GeneRows g = gene_rows(ctx, *p);
        std::vector<int32_t> rows((size_t)S);                                          // (the byte matrix is a host row store: row i is row i)
        for (int i = 0; i < S; i++) rows[(size_t)i] = g.rows ? g.rows[(size_t)perm[(size_t)i]] : perm[(size_t)i];
        if (gauss_gene_sumchi2_rows(ctx, mode, g.store, g.ld, g.format, rows.data(), S, p->pop_off.data(), g.pop_src_off, p->pop_wgt.data(),
                                    (int)p->pop_off.size() - 1, p->gene_off.data(), ng, g.on_device, z.data(), 1, r2, kept.data(), n_kept.data(),
                                    lam.data(), q.data(), top.data(), status.data(), nullptr) != 0) return herr("%s", gauss_last_error());
    }
    *out = sumchi2_output(geneid, p->gene_off, rsid, z, n_kept.data(), lam.data(), q.data(), top.data(), status.data());
    return 0;
}

int gauss_host_sumchi2(gauss_ctx* ctx, const char* study_pop, const char* input_file, const char* annotation_file,
                       const char* reference_index_file, const char* reference_data_file, const char* reference_pop_desc_file,
                       double af1_cutoff, double prune_r2, gauss_table** out)
{
    return run_sumchi2(ctx, call_gene(GAUSS_KIND_JEPEG, study_pop, nullptr, nullptr, 0, input_file, reference_index_file, reference_data_file,
                                      reference_pop_desc_file, af1_cutoff), annotation_file, prune_r2, out);
}

int gauss_host_sumchi2mix(gauss_ctx* ctx, const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                          const char* input_file, const char* annotation_file, const char* reference_index_file,
                          const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff,
                          double prune_r2, gauss_table** out)
{
    return run_sumchi2(ctx, call_gene(GAUSS_KIND_JEPEGMIX, nullptr, pop_names, pop_wgts, n_pop_wgt, input_file, reference_index_file,
                                      reference_data_file, reference_pop_desc_file, af1_cutoff), annotation_file, prune_r2, out);
}

int gauss_host_sumchi2_pval(const double* lam, int n, double q, double* p, int* n_pos)
{
    if (!lam || n < 0 || !p) return herr("bad arguments to gauss_host_sumchi2_pval");
    *p = sumchi2_pval(lam, n, q, n_pos);
    return 0;
}

int gauss_host_jepeg_rank(gauss_ctx* ctx, int kind, const char* study_pop, const char* const* pop_names, const double* pop_wgts,
                          int n_pop_wgt, const char* input_file, const char* annotation_file, const char* reference_index_file,
                          const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff,
                          int rank, int world, gauss_table** out)
{
    if (kind != GAUSS_KIND_JEPEG && kind != GAUSS_KIND_JEPEGMIX) return herr("kind %d is not jepeg / jepegmix", kind);
    return run_jepeg(ctx, call_gene(kind, study_pop, pop_names, pop_wgts, n_pop_wgt, input_file, reference_index_file, reference_data_file,
                                    reference_pop_desc_file, af1_cutoff), annotation_file, rank, world, out);
}

// Which rank runs which of n independent calls: longest first by `cost` onto the least loaded rank (ties: the lower index / rank).
static void deal_calls(const std::vector<double>& cost, int world, std::vector<int>& owner)
{
    const int n = (int)cost.size();
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cost[(size_t)x] > cost[(size_t)y]; });
    std::vector<double> load((size_t)std::max(1, world), 0.0);
    owner.assign((size_t)n, 0);
    for (int i : order) {
        int best = 0;
        for (int r = 1; r < world; r++) if (load[(size_t)r] < load[(size_t)best]) best = r;
        owner[(size_t)i] = best;
        load[(size_t)best] += cost[(size_t)i];
    }
}

int gauss_host_jepeg_genome(gauss_ctx* ctx, int kind, int n_calls, const char* study_pop, const char* const* pop_names,
                            const double* pop_wgts, int n_pop_wgt, const char* const* input_files, const char* const* annotation_files,
                            const char* const* reference_index_files, const char* const* reference_data_files,
                            const char* reference_pop_desc_file, double af1_cutoff, int rank, int world, gauss_table** out,
                            int32_t* owner_out)
{
    if (!ctx || !out || n_calls < 0 || !input_files || !annotation_files || !reference_data_files) return herr("bad arguments");
    if (kind != GAUSS_KIND_JEPEG && kind != GAUSS_KIND_JEPEGMIX) return herr("kind %d is not jepeg / jepegmix", kind);
    if (world < 1 || rank < 0 || rank >= world) return herr("rank %d of world %d", rank, world);
    // a call's cost: the size of its annotation file (its genes and gene SNPs are lines of it); every rank sees the same files
    std::vector<double> cost((size_t)n_calls, 1.0);
    for (int c = 0; c < n_calls; c++) {
        struct stat sb;
        if (annotation_files[c] && stat(annotation_files[c], &sb) == 0) cost[(size_t)c] = 1.0 + (double)sb.st_size;
    }
    std::vector<int> owner;
    deal_calls(cost, world, owner);
    int rc_all = 0;
    std::string first_err;
    for (int c = 0; c < n_calls; c++) {
        out[c] = nullptr;
        if (owner_out) owner_out[c] = owner[(size_t)c];
        if (owner[(size_t)c] != rank) continue;
        const char* idx = reference_index_files ? reference_index_files[c] : "(packed)";
        if (run_jepeg(ctx, call_gene(kind, study_pop, pop_names, pop_wgts, n_pop_wgt, input_files[c], idx ? idx : "(packed)", reference_data_files[c],
                                     reference_pop_desc_file, af1_cutoff), annotation_files[c], 0, 1, &out[c]) != 0) {
            // a call that fails leaves out[c] = NULL; the others still run (as the chromosome driver isolates a failing window)
            if (!rc_all) first_err = gauss_host_last_error();
            rc_all = -1;
            out[c] = nullptr;
        }
    }
    if (rc_all) return herr("%s", first_err.c_str());
    return 0;
}


}  // extern "C"
