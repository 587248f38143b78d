// libgauss_host.so -- result tables (the reference's output lists: dist.cpp:91-124, qcat.cpp:94-131, prep_qcat.cpp:135-204),
// the JEPEG k x k tail (gene.cpp:88-185, 317-550) and the table accessors of the C ABI (include/gauss_host.h).
#include <array>
#include "host_internal.h"

thread_local std::string g_err;

int herr(const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

// ------------------------------------------------------------------------------------------
// small dense helpers for the JEPEG k x k tail (k <= 6): gene.cpp:317-550
// ------------------------------------------------------------------------------------------
double pnorm_upper(double x) { return 0.5 * erfc(x / 1.4142135623730951); }   // R::pnorm5(x,0,1,0,0)

double pchisq_upper(double x, int df)                                            // R::pchisq(x,df,0,0)
{
    if (df <= 0) return NAN;
    if (!(x > 0.0)) return (x != x) ? NAN : 1.0;
    const double h = 0.5 * x;
    if ((df & 1) == 0) {
        double term = 1.0, sum = 1.0;
        for (int k = 1; k < df / 2; k++) { term *= h / k; sum += term; }
        return exp(-h) * sum;
    }
    double q = erfc(sqrt(h));
    if (df > 1) {
        double term = sqrt(h) / 0.886226925452758, sum = term;
        for (int k = 2; k <= (df - 1) / 2; k++) { term *= h / (k - 0.5); sum += term; }
        q += exp(-h) * sum;
    }
    return q;
}

// cyclic Jacobi for symmetric k x k (k <= 6); V columns are eigenvectors
static void jacobi_small(int n, double* A, double* V, double* d)
{
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) V[i * n + j] = (i == j);
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0;
        for (int i = 0; i < n; i++) for (int j = i + 1; j < n; j++) off += A[i * n + j] * A[i * n + j];
        if (off < 1e-300) break;
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; k++) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq; A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; k++) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk; A[q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; k++) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq; V[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < n; i++) d[i] = A[i * n + i];
}

static void make_pos_def_small(int n, double* M, double min_abs_eig)      // util.cpp:302-318
{
    double A[36], V[36], d[6];
    memcpy(A, M, sizeof(double) * n * n);
    jacobi_small(n, A, V, d);
    double mn = d[0];
    for (int i = 1; i < n; i++) mn = std::min(mn, d[i]);
    if (!(mn < min_abs_eig)) return;
    for (int i = 0; i < n; i++) if (d[i] < min_abs_eig) d[i] = min_abs_eig;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            double s = 0;
            for (int k = 0; k < n; k++) s += V[i * n + k] * d[k] * V[j * n + k];
            M[i * n + j] = s;
        }
}

static void inv_small(int n, const double* Min, double* inv)               // util.cpp:298-300 (full pivoting)
{
    double A[36];
    int rp[6], cp[6];
    memcpy(A, Min, sizeof(double) * n * n);
    for (int k = 0; k < n; k++) {
        int pi = k, pj = k; double best = -1;
        for (int i = k; i < n; i++) for (int j = k; j < n; j++) if (fabs(A[i * n + j]) > best) { best = fabs(A[i * n + j]); pi = i; pj = j; }
        rp[k] = pi; cp[k] = pj;
        if (pi != k) for (int j = 0; j < n; j++) std::swap(A[k * n + j], A[pi * n + j]);
        if (pj != k) for (int i = 0; i < n; i++) std::swap(A[i * n + k], A[i * n + pj]);
        for (int i = k + 1; i < n; i++) A[i * n + k] /= A[k * n + k];
        for (int i = k + 1; i < n; i++) for (int j = k + 1; j < n; j++) A[i * n + j] -= A[i * n + k] * A[k * n + j];
    }
    for (int c = 0; c < n; c++) {
        double col[6];
        for (int i = 0; i < n; i++) col[i] = (i == c);
        for (int k = 0; k < n; k++) if (rp[k] != k) std::swap(col[k], col[rp[k]]);
        for (int k = 0; k < n; k++) for (int i = k + 1; i < n; i++) col[i] -= A[i * n + k] * col[k];
        for (int k = n - 1; k >= 0; k--) { col[k] /= A[k * n + k]; for (int i = 0; i < k; i++) col[i] -= A[i * n + k] * col[k]; }
        for (int k = n - 1; k >= 0; k--) if (cp[k] != k) std::swap(col[k], col[cp[k]]);
        for (int i = 0; i < n; i++) inv[i * n + c] = col[i];
    }
}


static const char* categ_name(int c)       // Categ::GetName, gene.cpp:17-33
{
    static const char* nm[6] = {"PFS", "TFB", "STR", "TAR", "CIS", "TRN"};
    return (c >= 0 && c < 6) ? nm[c] : "";
}

// Gene::RunJepeg + CalJepegPval tail (gene.cpp:88-185, 317-550) given CorG (n x n row-major)
GeneResult jepeg_tail(const std::vector<Snp*>& gs, const double* CorG, const Args& a)
{
    GeneResult r;
    const int n = (int)gs.size();
    r.num_snp = n;
    int count[6] = {0, 0, 0, 0, 0, 0};
    for (Snp* s : gs) for (auto& kv : s->categ) if (kv.first >= 0 && kv.first < 6) count[kv.first]++;
    int cat[6], k = 0;
    for (int c = 0; c < 6; c++) if (count[c]) cat[k++] = c;
    if (n == 0 || k == 0) return r;
    std::vector<double> W((size_t)k * n), WC((size_t)k * n);
    for (int s = 0; s < n; s++)
        for (int i = 0; i < k; i++) {
            auto it = gs[s]->categ.find(cat[i]);
            const double w = (it != gs[s]->categ.end()) ? it->second : 0.0;     // Snp::GetCategWgt
            W[(size_t)i * n + s] = w * sqrt(gs[s]->info);                       // gene.cpp:871
        }
    double WWt[36], CovU[36], CorU[36], U[6], pv[6]; bool rmv[6];
    for (int i = 0; i < k; i++) for (int j = 0; j < k; j++) {
        double s = 0; for (int t = 0; t < n; t++) s += W[(size_t)i * n + t] * W[(size_t)j * n + t];
        WWt[i * k + j] = s;
    }
    for (int i = 0; i < k; i++) for (int s = 0; s < n; s++) {
        double v = 0; for (int t = 0; t < n; t++) v += W[(size_t)i * n + t] * CorG[(size_t)t * n + s];
        WC[(size_t)i * n + s] = v;
    }
    for (int i = 0; i < k; i++) for (int j = 0; j < k; j++) {
        double s = 0; for (int t = 0; t < n; t++) s += WC[(size_t)i * n + t] * W[(size_t)j * n + t];
        CovU[i * k + j] = s;
    }
    for (int i = 0; i < k; i++) for (int j = i; j < k; j++) {          // CnvrtCovToCor, util.cpp:284-296
        const double c = CovU[i * k + j] / (sqrt(CovU[i * k + i]) * sqrt(CovU[j * k + j]));
        CorU[i * k + j] = c; CorU[j * k + i] = c;
    }
    for (int i = 0; i < k; i++) {
        double s = 0; for (int t = 0; t < n; t++) s += W[(size_t)i * n + t] * gs[t]->z;
        U[i] = s;
        pv[i] = 2 * pnorm_upper(fabs(U[i] / sqrt(CovU[i * k + i])));      // gene.cpp:372-377
        rmv[i] = false;
    }
    for (int j = k - 1; j > 0; j--)                                      // gene.cpp:391-399
        for (int i = 0; i < j; i++) if (fabs(CorU[i * k + j]) > a.categ_cor_cutoff) { rmv[j] = true; break; }
    for (int i = 0; i < k; i++) if (CovU[i * k + i] < WWt[i * k + i] / a.denorm_norm_w) rmv[i] = true;   // gene.cpp:408-414
    int df = 0;
    for (int i = 0; i < k; i++) if (!rmv[i]) df++;
    r.df = df;
    if (!df) return r;
    double X[6], CovX[36], Inv[36];
    int ii = 0;
    for (int i = 0; i < k; i++) if (!rmv[i]) X[ii++] = U[i];
    int nn = 0;
    for (int i = 0; i < k; i++) { if (rmv[i]) continue; int mm = 0; for (int j = 0; j < k; j++) { if (rmv[j]) continue; CovX[nn * df + mm] = CovU[i * k + j]; mm++; } nn++; }
    make_pos_def_small(df, CovX, a.min_abs_eig);                        // gene.cpp:493
    inv_small(df, CovX, Inv);                                           // gene.cpp:494
    double cs = 0;
    for (int c = 0; c < df; c++) { double t = 0; for (int q = 0; q < df; q++) t += X[q] * Inv[q * df + c]; cs += t * X[c]; }
    r.chisq = cs;
    r.jepeg_pval = pchisq_upper(cs, df);                                // gene.cpp:509
    int top = 0;                                                        // GetTopCateg, gene.cpp:880-891
    for (int i = 0; i < k; i++) if ((pv[top] > pv[i]) & !rmv[i]) top = i;
    r.top_categ = categ_name(cat[top]);
    r.top_categ_pval = pv[top];
    int ts = 0;                                                         // GetTopSNP, gene.cpp:894-904
    for (int i = 0; i < n; i++) if (fabs(gs[ts]->z) < fabs(gs[i]->z)) ts = i;
    r.top_snp = gs[ts]->rsid;
    r.top_snp_pval = 2 * pnorm_upper(fabs(gs[ts]->z));
    r.geneid = gs[0]->geneid;                                           // gene.cpp:524 (only when df > 0)
    return r;
}

// ------------------------------------------------------------------------------------------
// outputs
// ------------------------------------------------------------------------------------------
// the SNPs of the prediction window, snp_vec order: what dist / qcat list (dist.cpp:92, qcat.cpp:95)
static std::vector<Snp*> window_rows(const gauss_prepared& p)
{
    std::vector<Snp*> rows;
    for (Snp* s : p.snp_vec) { const int ibp = (int)s->bp; if (ibp >= p.args.start_bp && ibp <= p.args.end_bp) rows.push_back(s); }
    return rows;
}

// (columns are filled in place, reserved to the row count: a chromosome's tables are 92 000 rows)
gauss_table* dist_output(gauss_prepared& p)     // dist.cpp:91-124 / distmix.cpp:100-133
{
    const bool mix = p.kind == GAUSS_KIND_DISTMIX;
    gauss_table* t = new gauss_table();
    const std::vector<Snp*> rows = window_rows(p);
    add_ident_columns(*t, rows);
    Column &af = t->add(mix ? "af1mix" : "af1ref", GAUSS_COL_DBL), &z = t->add("z", GAUSS_COL_DBL), &pval = t->add("pval", GAUSS_COL_DBL);
    Column &info = t->add("info", GAUSS_COL_DBL), &type = t->add("type", GAUSS_COL_INT);
    for (Column* c : {&af, &z, &pval, &info}) c->d.reserve(rows.size());
    type.i.reserve(rows.size());
    for (Snp* s : rows) {
        af.d.push_back(mix ? s->af1mix : s->af1ref);
        z.d.push_back(s->z);
        pval.d.push_back(2 * pnorm_upper(fabs(s->z)));            // dist.cpp:101
        info.d.push_back(s->info); type.i.push_back(s->type);
    }
    return t;
}

// rsid chr bp a1 a2 af1ref|af1mix z z_loo info_loo t pval: the measured SNPs of the prediction window, each re-imputed from the
// other measured SNPs of the extended window; pval = 2 pnorm(-|t|) of the standardised residual
gauss_table* loo_output(bool mix, const std::vector<LooRow>& rows, const double* loo_z, const double* loo_info, const double* loo_t)
{
    gauss_table* t = new gauss_table();
    add_ident_columns(*t, rows.size(), [&](size_t i) { return rows[i].id; });
    Column &af = t->add(mix ? "af1mix" : "af1ref", GAUSS_COL_DBL), &z = t->add("z", GAUSS_COL_DBL), &zl = t->add("z_loo", GAUSS_COL_DBL);
    Column &il = t->add("info_loo", GAUSS_COL_DBL), &tt = t->add("t", GAUSS_COL_DBL), &pval = t->add("pval", GAUSS_COL_DBL);
    for (Column* c : {&af, &z, &zl, &il, &tt, &pval}) c->d.reserve(rows.size());
    for (const LooRow& r : rows) {
        af.d.push_back(r.af); z.d.push_back(r.z);
        zl.d.push_back(loo_z[r.idx]); il.d.push_back(loo_info[r.idx]); tt.d.push_back(loo_t[r.idx]);
        pval.d.push_back(2 * pnorm_upper(fabs(loo_t[r.idx])));
    }
    return t;
}

// rsid chr bp a1 a2 af1ref|af1mix z wing order z_entry z_joint z_cond pval_cond var_left: every measured SNP of the extended window
// (wing = 1 outside the prediction window: a signal in a wing is conditioned on, not hidden); order = 1 .. n for the selected SNPs in
// order of entry, 0 otherwise; z_entry / z_joint NaN unless selected; pval_cond = 2 pnorm(-|z_cond|)
gauss_table* slct_output(bool mix, const std::vector<ViewSnp>& rows, int n_sel, const int32_t* idx, const double* zin, const double* joint,
                         const double* zc, const double* var_left)
{
    gauss_table* t = new gauss_table();
    add_ident_columns(*t, rows.size(), [&](size_t i) { return rows[i].id; });
    Column &af = t->add(mix ? "af1mix" : "af1ref", GAUSS_COL_DBL), &z = t->add("z", GAUSS_COL_DBL), &wing = t->add("wing", GAUSS_COL_INT);
    Column &order = t->add("order", GAUSS_COL_INT), &ze = t->add("z_entry", GAUSS_COL_DBL), &zj = t->add("z_joint", GAUSS_COL_DBL);
    Column &zcond = t->add("z_cond", GAUSS_COL_DBL), &pval = t->add("pval_cond", GAUSS_COL_DBL), &vl = t->add("var_left", GAUSS_COL_DBL);
    std::vector<int> ord(rows.size(), 0);
    for (int a = 0; a < n_sel; a++) ord[(size_t)idx[a]] = a + 1;
    for (size_t i = 0; i < rows.size(); i++) {
        const int o = ord[i];
        af.d.push_back(rows[i].af); z.d.push_back(rows[i].z); wing.i.push_back(rows[i].wing); order.i.push_back(o);
        ze.d.push_back(o ? zin[o - 1] : NAN); zj.d.push_back(o ? joint[o - 1] : NAN);
        zcond.d.push_back(zc[i]); pval.d.push_back(2 * pnorm_upper(fabs(zc[i]))); vl.d.push_back(var_left[i]);
    }
    return t;
}

// dist_cond / distmix_cond: `t` is dist_output's table of the same call (the SNPs of the prediction window, untouched); the measured SNPs
// of the wings follow it in matrix order (info 1, type 1 like every measured SNP), so that every selected SNP has a row; then the
// selection's columns wing order z_cond pval_cond var_left are added: a measured row carries what slct_output gives it, an imputed
// row the statistics conditioned on the selected SNPs and order 0.  z_entry / z_joint of the n selected SNPs go to the named
// matrix `signals` [n x 3]: table row (from 0), z_entry, z_joint, in order of entry.  Returns 0, or -1 with the message set when `t`
// holds a column this function does not know how to fill for a wing row (`t` is then left as it came).
// The measured SNPs the call's own table does not list (the wings': row_m < 0) appended to it in matrix order, so that every measured SNP
// has a row: `at` = table row of measured SNP i, `nrow` = rows afterwards.  `room` further columns must still fit.  -1: message set
static int append_wing_rows(gauss_table& t, const std::vector<ViewSnp>& rows, const std::vector<int32_t>& row_m, size_t room, const char* who,
                            std::vector<int32_t>& at, size_t& nrow)
{
    static const char* const known[] = {"rsid", "chr", "bp", "a1", "a2", "af1ref", "af1mix", "z", "pval", "info", "type"};
    for (const Column& c : t.cols)
        if (std::none_of(std::begin(known), std::end(known), [&](const char* k) { return c.name == k; }))
            return herr("%s: no value for column '%s' in the rows of the wings", who, c.name.c_str());
    if (t.cols.size() + room > (size_t)gauss_table::MAX_COLS) return herr("%s: %zu columns leave no room for %zu more", who, t.cols.size(), room);
    nrow = (size_t)t.nrow();
    at = row_m;                                                       // table row of measured SNP i, the appended ones included
    for (size_t i = 0; i < rows.size(); i++) {
        if (at[i] >= 0) continue;
        at[i] = (int32_t)nrow++;
        const ViewSnp& r = rows[i];
        for (Column& c : t.cols) {
            if (c.name == "rsid") c.s.emplace_back(r.id.rsid);
            else if (c.name == "a1") c.s.emplace_back(r.id.a1);
            else if (c.name == "a2") c.s.emplace_back(r.id.a2);
            else if (c.name == "chr") c.i.push_back(r.id.chr);
            else if (c.name == "bp") c.i.push_back((int)r.id.bp);
            else if (c.name == "type") c.i.push_back(1);
            else if (c.name == "z") c.d.push_back(r.z);
            else if (c.name == "pval") c.d.push_back(2 * pnorm_upper(fabs(r.z)));
            else if (c.name == "info") c.d.push_back(1.0);
            else c.d.push_back(r.af);                                 // af1ref | af1mix: the names were checked above
        }
    }
    return 0;
}

int cond_output(gauss_table& t, const std::vector<ViewSnp>& rows, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u,
                 int n_sel, const int32_t* idx, const double* zin, const double* joint, const double* zc, const double* var_left,
                 const double* cond_z, const double* cond_var)
{
    std::vector<int32_t> at;
    size_t nrow = 0;
    if (append_wing_rows(t, rows, row_m, 5, "cond_output", at, nrow)) return -1;
    Column &wing = t.add("wing", GAUSS_COL_INT), &order = t.add("order", GAUSS_COL_INT), &zcond = t.add("z_cond", GAUSS_COL_DBL);
    Column &pval = t.add("pval_cond", GAUSS_COL_DBL), &vl = t.add("var_left", GAUSS_COL_DBL);
    wing.i.assign(nrow, 0); order.i.assign(nrow, 0);
    zcond.d.assign(nrow, NAN); pval.d.assign(nrow, NAN); vl.d.assign(nrow, NAN);
    for (size_t i = 0; i < rows.size(); i++) {
        const size_t r = (size_t)at[i];
        wing.i[r] = rows[i].wing; zcond.d[r] = zc[i]; vl.d[r] = var_left[i];
    }
    for (size_t u = 0; u < row_u.size(); u++) {
        if (row_u[u] < 0) continue;
        zcond.d[(size_t)row_u[u]] = cond_z[u]; vl.d[(size_t)row_u[u]] = cond_var[u];
    }
    for (size_t r = 0; r < nrow; r++) pval.d[r] = 2 * pnorm_upper(fabs(zcond.d[r]));
    std::vector<double> sig((size_t)n_sel * 3);
    for (int a = 0; a < n_sel; a++) {
        const int32_t r = at[(size_t)idx[a]];
        order.i[(size_t)r] = a + 1;
        sig[(size_t)a] = (double)r; sig[(size_t)n_sel + a] = zin[a]; sig[2 * (size_t)n_sel + a] = joint[a];
    }
    t.put_named("signals", n_sel, 3, std::move(sig));
    return 0;
}

// dist_cs / distmix_cs: `t` is cond_output's table of the same call -- dist_output's rows, then the wings' measured SNPs in matrix order,
// which is how the table row of a measured SNP the plain table does not list is found again.  Adds pip, cs (1-based order of entry of
// the set that holds the SNP, 0: none) and cs_pip, and the named matrix `sets` [n x 4]: table row of the lead SNP, size, mass, lse.
int cs_output(gauss_table& t, const std::vector<ViewSnp>& rows, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u,
              int n_sel, const int32_t* idx, const double* pip, const int32_t* set, const double* set_pip,
              const int32_t* size, const double* mass, const double* lse)
{
    size_t listed = 0, wings = 0;
    for (int32_t r : row_m) (r >= 0 ? listed : wings)++;
    for (int32_t r : row_u) if (r >= 0) listed++;
    const size_t nrow = (size_t)t.nrow(), M = rows.size();
    if (t.cols.empty() || t.cols.back().name != "var_left" || row_m.size() != M || nrow < wings)
        return herr("cs_output: the table is not the conditional one of the same window");
    std::vector<int32_t> at(row_m);                                   // cond_output's rows: the wings' SNPs follow the plain table
    int32_t next = (int32_t)(nrow - wings);
    for (size_t i = 0; i < M; i++) if (at[i] < 0) at[i] = next++;
    t.widen(3);
    Column &p = t.add("pip", GAUSS_COL_DBL), &cs = t.add("cs", GAUSS_COL_INT), &cp = t.add("cs_pip", GAUSS_COL_DBL);
    p.d.assign(nrow, NAN); cs.i.assign(nrow, 0); cp.d.assign(nrow, NAN);
    auto put = [&](int32_t r, size_t c) {
        if (r < 0) return;
        p.d[(size_t)r] = pip[c]; cs.i[(size_t)r] = set[c] + 1; cp.d[(size_t)r] = set_pip[c];
    };
    for (size_t i = 0; i < M; i++) put(at[i], i);
    for (size_t u = 0; u < row_u.size(); u++) put(row_u[u], M + u);
    std::vector<double> sets((size_t)n_sel * 4);
    for (int a = 0; a < n_sel; a++) {
        sets[(size_t)a] = (double)at[(size_t)idx[a]]; sets[(size_t)n_sel + a] = (double)size[a];
        sets[2 * (size_t)n_sel + a] = mass[a]; sets[3 * (size_t)n_sel + a] = lse[a];
    }
    t.put_named("sets", n_sel, 4, std::move(sets));
    return 0;
}

// dist_susie / distmix_susie: `t` is the call's own table.  The wings' measured SNPs are appended as cond_output appends them; adds
// wing, pip, cs (1-based effect of the kept set that holds the SNP, 0: none) and cs_pip, the named matrices `effects` [L x 7] (table row
// of the SNP of largest alpha, V, lse, size, mass, purity, kept) and `fit` [1 x 3] (sweeps, delta, converged), and a message when the
// sweeps ran out or the window was not fitted
// One trait's fit in the table: the columns pip<cs> cs<cs> cs_pip<cs> by candidate (row_of[c]: the candidate's table row, -1: not listed),
// the named matrices effects<nm> and fit<nm>, and a message (`who` names the trait) when the sweeps ran out or nothing was fitted
static void susie_trait_output(gauss_table& t, size_t nrow, const std::vector<int32_t>& row_of, const std::string& cs_sfx, const std::string& nm_sfx,
                               const std::string& who, int L, double tol, const double* pip, const int32_t* set, const double* set_pip,
                               const double* alpha, const double* V, const double* lse, const int32_t* size, const double* mass,
                               const double* purity, const int32_t* kept, const double* sweeps)
{
    const size_t T = row_of.size();
    Column &p = t.add(("pip" + cs_sfx).c_str(), GAUSS_COL_DBL), &cs = t.add(("cs" + cs_sfx).c_str(), GAUSS_COL_INT),
           &cp = t.add(("cs_pip" + cs_sfx).c_str(), GAUSS_COL_DBL);
    p.d.assign(nrow, NAN); cs.i.assign(nrow, 0); cp.d.assign(nrow, NAN);
    for (size_t c = 0; c < T; c++) {
        if (row_of[c] < 0) continue;
        const size_t r = (size_t)row_of[c];
        p.d[r] = pip[c]; cs.i[r] = set[c] + 1; cp.d[r] = set_pip[c];
    }
    const bool fitted = sweeps[0] > 0;
    std::vector<double> eff((size_t)L * 7);
    for (int l = 0; l < L; l++) {
        int32_t lead = -1;
        if (fitted) {
            size_t best = 0;
            for (size_t c = 1; c < T; c++) if (alpha[(size_t)l * T + c] > alpha[(size_t)l * T + best]) best = c;
            lead = row_of[best];
        }
        const double vals[7] = {(double)lead, V[l], lse[l], (double)size[l], mass[l], purity[l], (double)kept[l]};
        for (int k = 0; k < 7; k++) eff[(size_t)k * L + l] = vals[k];
    }
    t.put_named(("effects" + nm_sfx).c_str(), L, 7, std::move(eff));
    // tol = 0 (the caller asked for exactly max_sweeps sweeps with a negative tol): delta < 0 never holds, so `converged` is 0, and
    // running the sweeps out is what was asked for: no message
    const bool converged = fitted && sweeps[1] < tol;
    t.put_named(("fit" + nm_sfx).c_str(), 1, 3, std::vector<double>{sweeps[0], sweeps[1], converged ? 1.0 : 0.0});
    if (!fitted) t.messages.push_back(who + ": the window was not fitted (its B11 is not finite, or MakePosDef repaired it): pip, cs and cs_pip are empty");
    else if (!converged && tol > 0) t.messages.push_back(who + ": the sweeps ran out before the fit converged (max_sweeps); the values are those of the last sweep");
}

// the wing column and the table row of every candidate, the measured SNPs (appended ones included) first
static std::vector<int32_t> wing_column(gauss_table& t, size_t nrow, const std::vector<ViewSnp>& rows, const std::vector<int32_t>& at,
                                        const std::vector<int32_t>& row_u)
{
    const size_t M = rows.size();
    Column& wing = t.add("wing", GAUSS_COL_INT);
    wing.i.assign(nrow, 0);
    std::vector<int32_t> row_of(M + row_u.size(), -1);
    for (size_t i = 0; i < M; i++) { row_of[i] = at[i]; wing.i[(size_t)at[i]] = rows[i].wing; }
    for (size_t u = 0; u < row_u.size(); u++) row_of[M + u] = row_u[u];
    return row_of;
}

int susie_output(gauss_table& t, const std::vector<ViewSnp>& rows, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u,
                 int L, double tol, const double* pip, const int32_t* set, const double* set_pip, const double* alpha, const double* V,
                 const double* lse, const int32_t* size, const double* mass, const double* purity, const int32_t* kept, const double* sweeps)
{
    std::vector<int32_t> at;
    size_t nrow = 0;
    if (append_wing_rows(t, rows, row_m, 4, "susie_output", at, nrow)) return -1;
    const std::vector<int32_t> row_of = wing_column(t, nrow, rows, at, row_u);
    susie_trait_output(t, nrow, row_of, "", "", "susie", L, tol, pip, set, set_pip, alpha, V, lse, size, mass, purity, kept, sweeps);
    return 0;
}

int xs_build_map(const int64_t* key_lead, size_t n_lead, const int64_t* key_peer, size_t n_peer, int32_t* from_lead)
{
    std::map<int64_t, int32_t> at;
    for (size_t c = 0; c < n_peer; c++)
        if (!at.emplace(key_peer[c], (int32_t)c).second)
            return herr("xs_build_map: candidates %d and %zu of a study are the same panel SNP", (int)at[key_peer[c]], c);
    std::map<int64_t, int32_t> seen;
    int shared = 0;
    for (size_t j = 0; j < n_lead; j++) {
        if (!seen.emplace(key_lead[j], (int32_t)j).second)
            return herr("xs_build_map: candidates %d and %zu of the first study are the same panel SNP", (int)seen[key_lead[j]], j);
        const auto it = at.find(key_lead[j]);
        from_lead[j] = it == at.end() ? -1 : it->second;
        shared += it == at.end() ? 0 : 1;
    }
    return shared;
}

int xsusie_output(gauss_table& t, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u, const uint8_t* joint, int K, int L,
                  const double* xs_V, const double* xs_purity, const int32_t* status)
{
    size_t wings = 0;
    for (int32_t r : row_m) wings += r < 0 ? 1 : 0;
    const size_t nrow = (size_t)t.nrow(), M = row_m.size();
    NamedMat* eff = nullptr;
    for (NamedMat& m : t.named) if (m.name == "effects") eff = &m;
    if (nrow < wings || !eff || eff->nrow != L || eff->ncol != 7) return herr("xsusie_output: the table is not susie_output's of the same window");
    Column& jc = t.add("joint", GAUSS_COL_INT);
    jc.i.assign(nrow, 0);
    int32_t next = (int32_t)(nrow - wings);                            // susie_output's rows: the wings' SNPs follow the call's own
    for (size_t i = 0; i < M; i++) jc.i[(size_t)(row_m[i] >= 0 ? row_m[i] : next++)] = joint[i] ? 1 : 0;
    for (size_t u = 0; u < row_u.size(); u++) if (row_u[u] >= 0) jc.i[(size_t)row_u[u]] = joint[M + u] ? 1 : 0;
    const size_t l = (size_t)L, nc = 2 * (size_t)K + 5;
    std::vector<double> e(l * nc), old(eff->d);                       // old, column-major: row, V, lse, size, mass, purity, kept
    for (size_t a = 0; a < l; a++) {
        e[a] = old[a];
        for (int k = 0; k < K; k++) { e[(1 + (size_t)k) * l + a] = xs_V[(size_t)k * l + a]; e[(1 + (size_t)K + k) * l + a] = xs_purity[(size_t)k * l + a]; }
        e[(2 * (size_t)K + 1) * l + a] = old[2 * l + a]; e[(2 * (size_t)K + 2) * l + a] = old[3 * l + a];
        e[(2 * (size_t)K + 3) * l + a] = old[4 * l + a]; e[(2 * (size_t)K + 4) * l + a] = old[6 * l + a];
    }
    eff->ncol = (int)nc; eff->d = std::move(e);
    for (int k = 0; k < K; k++)
        if (status[k] & (GAUSS_ST_CLAMPED | GAUSS_ST_NONFINITE))
            t.messages.push_back("xsusie: the group was not fitted: the B11 of study " + std::to_string(k + 1) +
                                 (status[k] & GAUSS_ST_NONFINITE ? " is not finite" : " was repaired by MakePosDef"));
    return 0;
}

int coloc_output(gauss_table& t, const std::vector<ViewSnp>& rows, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u,
                 int L, double tol, const SusieFit& first, int n_more, const double* z_more, const double* out_z_more, const ColocMore& more)
{
    std::vector<int32_t> at;
    size_t nrow = 0;
    if (append_wing_rows(t, rows, row_m, 4, "coloc_output", at, nrow)) return -1;
    const int k = more.k;
    t.widen(4 + 3 * (size_t)k);                                       // before the first add(): no reference into the table is held
    const std::vector<int32_t> row_of = wing_column(t, nrow, rows, at, row_u);
    const size_t Tn = row_of.size(), lt = (size_t)L * Tn;
    susie_trait_output(t, nrow, row_of, "", "_1", "coloc, trait 1", L, tol, first.pip, first.set, first.set_pip, first.alpha, first.V, first.lse,
                       first.size, first.mass, first.purity, first.kept, first.sweeps);
    for (int q = 0; q < k; q++) {
        const std::string n = std::to_string(q + 2);
        const SusieFit& f = more.fit;
        susie_trait_output(t, nrow, row_of, "_" + n, "_" + n, "coloc, trait " + n, L, tol, f.pip + q * Tn, f.set + q * Tn, f.set_pip + q * Tn,
                           f.alpha + q * lt, f.V + (size_t)q * L, f.lse + (size_t)q * L, f.size + (size_t)q * L, f.mass + (size_t)q * L,
                           f.purity + (size_t)q * L, f.kept + (size_t)q * L, f.sweeps + 2 * (size_t)q);
    }
    // the further traits' Z-scores on every row, the wings' measured SNPs included
    traits_output(t, n_more, at, row_u, z_more, out_z_more);
    // one row per pair of kept effects of two traits
    std::vector<std::array<double, 12>> out;
    size_t pair = 0;
    for (int a = 0; a <= k; a++)
        for (int b = a + 1; b <= k; b++, pair++)
            for (int la = 0; la < L; la++)
                for (int lb = 0; lb < L; lb++) {
                    const size_t e = (pair * L + la) * L + lb;
                    const int32_t hit = more.hit[e];
                    if (hit < 0) continue;
                    const double* pp = more.pp + 5 * e;
                    out.push_back({(double)(a + 1), (double)(b + 1), (double)(la + 1), (double)(lb + 1), (double)more.n[pair], pp[0], pp[1], pp[2],
                                   pp[3], pp[4], (double)((size_t)hit < Tn ? row_of[(size_t)hit] : -1), more.hit_pp[e]});
                }
    std::vector<double> cm(out.size() * 12);
    for (size_t r = 0; r < out.size(); r++)
        for (int c = 0; c < 12; c++) cm[(size_t)c * out.size() + r] = out[r][(size_t)c];
    t.put_named("coloc", (int)out.size(), 12, std::move(cm));
    return 0;
}

// dist_prs / distmix_prs: one row per measured SNP of the extended window; `beta` [n_s n_lam x rows] and `grid` [n_s n_lam x 9] as named
// matrices (host_internal.h).  converged = delta < tol r_max (or r_max = 0), the kernel's own rule on the same r
gauss_table* prs_output(bool mix, const std::vector<ViewSnp>& rows, double n, double tol, const std::vector<double>& s,
                        const std::vector<double>& lam, const double* beta, const int32_t* nnz, const int32_t* sweeps, const double* delta,
                        const double* br, const double* bg, const double* kkt)
{
    gauss_table* t = new gauss_table();
    add_ident_columns(*t, rows.size(), [&](size_t i) { return rows[i].id; });
    Column &af = t->add(mix ? "af1mix" : "af1ref", GAUSS_COL_DBL), &z = t->add("z", GAUSS_COL_DBL), &r = t->add("r", GAUSS_COL_DBL);
    Column& wing = t->add("wing", GAUSS_COL_INT);
    const size_t M = rows.size(), nl = lam.size(), nc = s.size() * nl;
    double rmax = 0.0;
    for (size_t i = 0; i < M; i++) {
        const double zi = rows[i].z;
        const double ri = std::isfinite(zi) ? zi / sqrt(n - 2.0 + zi * zi) : 0.0;
        af.d.push_back(rows[i].af); z.d.push_back(zi); r.d.push_back(ri); wing.i.push_back(rows[i].wing);
        rmax = std::max(rmax, fabs(ri));
    }
    std::vector<double> b(nc * M), g(nc * 9);
    bool ran_out = false, fitted = true;
    for (size_t c = 0; c < nc; c++) {
        for (size_t i = 0; i < M; i++) b[i * nc + c] = beta[c * M + i];
        const bool conv = sweeps[c] > 0 && (delta[c] < tol * rmax || rmax == 0.0);
        fitted = fitted && sweeps[c] > 0;
        ran_out = ran_out || (sweeps[c] > 0 && !conv);
        const double vals[9] = {s[c / nl], lam[c % nl], (double)nnz[c], (double)sweeps[c], delta[c], br[c], bg[c], kkt[c], conv ? 1.0 : 0.0};
        for (int k = 0; k < 9; k++) g[(size_t)k * nc + c] = vals[k];
    }
    t->put_named("beta", (int)nc, (int)M, std::move(b));
    t->put_named("grid", (int)nc, 9, std::move(g));
    if (!fitted) t->messages.push_back("prs: the window was not fitted (its B11 is not finite): the weights are empty");
    else if (ran_out) t->messages.push_back("prs: some (s, lam) ran its sweeps out before it converged (max_sweeps); its weights are those of the last sweep");
    return t;
}

// dist_ldscore / distmix_ldscore: one row per target (host_internal.h); n_band travels as the exact double the device summed
gauss_table* ldscore_output(bool mix, const std::vector<ViewSnp>& rows, const double* l2, const double* raw, const double* mass, double n_eff,
                            int64_t n_ref, int64_t n_ref_5_50, int64_t radius)
{
    gauss_table* t = new gauss_table();
    add_ident_columns(*t, rows.size(), [&](size_t i) { return rows[i].id; });
    Column &af = t->add(mix ? "af1mix" : "af1ref", GAUSS_COL_DBL), &c_l2 = t->add("l2", GAUSS_COL_DBL), &c_raw = t->add("l2_raw", GAUSS_COL_DBL);
    Column& band = t->add("n_band", GAUSS_COL_INT);
    bool nan = false;
    for (size_t i = 0; i < rows.size(); i++) {
        af.d.push_back(rows[i].af); c_l2.d.push_back(l2[i]); c_raw.d.push_back(raw[i]);
        band.i.push_back(mass[i] >= 0.0 && mass[i] <= (double)INT32_MAX ? (int)mass[i] : -1);      // (a count of rows; -1: not one, NaN included)
        nan = nan || raw[i] != raw[i];
    }
    t->put_named("ldscore", 1, 4, std::vector<double>{n_eff, (double)n_ref, (double)n_ref_5_50, (double)radius});
    if (nan) t->messages.push_back("ldscore: some scores are NaN: a panel SNP inside their band has no variance in the selected populations");
    return t;
}

double kish_n_eff(const double* w, const int32_t* pop_off, int P)
{
    double sw = 0.0, sq = 0.0;
    for (int p = 0; p < P; p++) {
        if (w[p] == 0.0) continue;
        sw += w[p];
        sq += w[p] * w[p] / (double)(pop_off[p + 1] - pop_off[p]);
    }
    return sw * sw / sq;
}

int traits_match(const GwasCache& gw, const char* path, size_t n, const std::function<SnpIdent(size_t)>& at, double* z_out,
                 uint8_t* miss_out, size_t* n_missing)
{
    size_t missing = 0;
    std::string first_missing;
    for (size_t i = 0; i < n; i++) {
        const SnpIdent s = at(i);
        auto before = [&](uint32_t x, long long bp) { const GwasRow& r = gw.rows[x]; return r.chr < s.chr || (r.chr == s.chr && r.bp < bp); };
        bool found = false;
        double z = 0.0;
        // the rows of one position keep their file order in by_pos: the last match is the later row
        for (auto it = std::lower_bound(gw.by_pos.begin(), gw.by_pos.end(), s.bp, before); it != gw.by_pos.end(); ++it) {
            const GwasRow& r = gw.rows[*it];
            if (r.chr != s.chr || r.bp != s.bp) break;
            if (r.a1 == s.a1 && r.a2 == s.a2) { z = r.z; found = true; }
            else if (r.a1 == s.a2 && r.a2 == s.a1) { z = -r.z; found = true; }        // gauss.cpp:358-370
        }
        if (miss_out) miss_out[i] = found ? 0 : 1;
        if (!found) { if (!missing++) first_missing = s.rsid; if (miss_out) z_out[i] = 0.0; continue; }
        if (!std::isfinite(z)) return herr("ERROR: %s: the z of %s is not finite", path, s.rsid);
        z_out[i] = z;
    }
    if (n_missing) *n_missing = missing;
    if (missing && !miss_out)
        return herr("ERROR: %s lacks %zu of the window's %zu measured SNPs, the first is %s: every trait must be measured at the SNPs of the first",
                    path, missing, n, first_missing.c_str());
    return 0;
}

int traits_miss_limits(const char* const* paths, int n_more, size_t M, const uint8_t* mask, int min_measured)
{
    std::vector<uint8_t> any(M, 0);
    for (int k = 0; k < n_more; k++) {
        size_t lacks = 0;
        for (size_t i = 0; i < M; i++) if (mask[(size_t)k * M + i]) { lacks++; any[i] = 1; }
        if (lacks > (size_t)GAUSS_TRAITS_MISS_MAX)
            return herr("ERROR: %s lacks %zu of the window's %zu measured SNPs: a trait may lack at most %d of them", paths[k], lacks, M, GAUSS_TRAITS_MISS_MAX);
        if (M - lacks <= (size_t)min_measured)
            return herr("ERROR: %s has %zu of the window's %zu measured SNPs: a trait needs more than %d", paths[k], M - lacks, M, min_measured);
    }
    const size_t distinct = (size_t)std::count(any.begin(), any.end(), (uint8_t)1);
    if (distinct > (size_t)GAUSS_TRAITS_MISS_UNION_MAX)
        return herr("ERROR: %zu distinct measured SNPs of the window are missing in one of the %d further files (the last is %s): a window takes at most %d",
                    distinct, n_more, paths[n_more - 1], GAUSS_TRAITS_MISS_UNION_MAX);
    return 0;
}

void traits_output(gauss_table& t, int n_more, const std::vector<int32_t>& row_m, const std::vector<int32_t>& row_u,
                   const double* z_more, const double* out_z_more, const TraitsMiss* miss)
{
    const size_t nrow = (size_t)t.nrow(), M = row_m.size(), U = row_u.size();
    std::vector<double> z(nrow * (size_t)(1 + n_more), NAN), pv(nrow * (size_t)(1 + n_more), NAN);
    for (const Column& c : t.cols) {
        if (c.name == "z") std::copy(c.d.begin(), c.d.end(), z.begin());
        if (c.name == "pval") std::copy(c.d.begin(), c.d.end(), pv.begin());
    }
    for (int k = 0; k < n_more; k++) {
        double* zc = z.data() + nrow * (size_t)(1 + k);
        double* pc = pv.data() + nrow * (size_t)(1 + k);
        for (size_t i = 0; i < M; i++) if (row_m[i] >= 0) zc[(size_t)row_m[i]] = z_more[(size_t)k * M + i];
        for (size_t i = 0; i < U; i++) if (row_u[i] >= 0) zc[(size_t)row_u[i]] = out_z_more[(size_t)k * U + i];
        for (size_t r = 0; r < nrow; r++) pc[r] = 2 * pnorm_upper(fabs(zc[r]));       // dist.cpp:101
    }
    std::vector<double> info, type, n_missing;
    if (miss) {
        // a present measured SNP and every SNP's type: as in the table's own columns (the same SNP, the same window)
        info.assign(nrow * (size_t)(1 + n_more), NAN); type = info;
        n_missing.assign((size_t)(1 + n_more), 0.0);
        for (const Column& c : t.cols) {
            if (c.name == "info") for (int k = 0; k <= n_more; k++) std::copy(c.d.begin(), c.d.end(), info.begin() + nrow * (size_t)k);
            if (c.name == "type") for (int k = 0; k <= n_more; k++) std::copy(c.i.begin(), c.i.end(), type.begin() + nrow * (size_t)k);
        }
        size_t at = 0;                                                 // z_miss / info_miss: one entry per set mask bit, in mask order
        for (int k = 0; k < n_more; k++) {
            const size_t col = nrow * (size_t)(1 + k);
            for (size_t i = 0; i < U; i++) if (row_u[i] >= 0) info[col + (size_t)row_u[i]] = miss->info_more[(size_t)k * U + i];
            for (size_t i = 0; i < M; i++) {
                if (!miss->mask[(size_t)k * M + i]) continue;
                n_missing[(size_t)(1 + k)] += 1.0;
                if (row_m[i] >= 0) {
                    const size_t r = col + (size_t)row_m[i];
                    z[r] = miss->z_miss[at]; pv[r] = 2 * pnorm_upper(fabs(z[r])); info[r] = miss->info_miss[at]; type[r] = 0.0;
                }
                at++;
            }
        }
    }
    t.put_named("z_traits", (int)nrow, 1 + n_more, std::move(z));
    t.put_named("pval_traits", (int)nrow, 1 + n_more, std::move(pv));
    if (miss) {
        t.put_named("info_traits", (int)nrow, 1 + n_more, std::move(info));
        t.put_named("type_traits", (int)nrow, 1 + n_more, std::move(type));
        t.put_named("n_missing", 1 + n_more, 1, std::move(n_missing));
    }
}

// Positive doubles order as their bit patterns do: bisection on the pattern ends at the last bit that changes the comparison.
double slct_chi2_of(double p)
{
    auto below = [&](double chi2) { return 2 * pnorm_upper(sqrt(chi2)) < p; };
    if (below(0.0)) return 0.0;                               // p > 1: everything passes
    double hi_d = 1e5;                                        // (erfc has underflowed to 0 long before: below(hi) holds for every p > 0)
    uint64_t lo = 0, hi;
    memcpy(&hi, &hi_d, sizeof(hi));
    while (hi - lo > 1) {                                     // invariant: !below(lo), below(hi)
        const uint64_t mid = lo + (hi - lo) / 2;
        double m;
        memcpy(&m, &mid, sizeof(m));
        if (below(m)) hi = mid; else lo = mid;
    }
    memcpy(&hi_d, &hi, sizeof(hi));
    return hi_d;
}

int clump_keys(double p1, double p2, double r2, double kb, ClumpKeys& out)
{
    const double a = std::isnan(p1) ? 1e-4 : p1, b = std::isnan(p2) ? 1e-2 : p2;                                 // PLINK's --clump-p1 / --clump-p2
    if (!(a > 0.0 && a <= 1.0)) return herr("clump: p1 = %g is outside (0, 1]", a);
    if (!(b > 0.0 && b <= 1.0)) return herr("clump: p2 = %g is outside (0, 1]", b);
    const double rr = std::isnan(r2) ? 0.5 : r2, k = std::isnan(kb) ? 250.0 : kb;                                // --clump-r2 / --clump-kb
    if (b < a) return herr("clump: p2 = %g is below p1 = %g (a member's threshold is no stricter than an index SNP's)", b, a);
    if (!(rr >= 0.0 && rr <= 1.0)) return herr("clump: r2 = %g is outside [0, 1]", rr);
    if (!(k >= 0.0) || !std::isfinite(k) || k * 1000.0 > 4e9) return herr("clump: kb = %g; the distance is 0 .. 4 000 000 kb", k);
    out.key_index = slct_chi2_of(a); out.key_member = slct_chi2_of(b); out.r2_min = rr;
    out.radius = (int64_t)llround(k * 1000.0);
    return 0;
}

void clump_output(gauss_table& t, const std::vector<double>& z, const int32_t* owner, const int32_t* rank, const double* r2, int n_clumps)
{
    const size_t M = z.size(), n = (size_t)std::max(n_clumps, 0);
    t.widen(5);                                                         // room for the five columns: no add() below moves a column
    Column &zc = t.add("z", GAUSS_COL_DBL), &pval = t.add("pval", GAUSS_COL_DBL), &clump = t.add("clump", GAUSS_COL_INT);
    Column &lead = t.add("index_rsid", GAUSS_COL_STR), &rc = t.add("r2", GAUSS_COL_DBL);
    const std::vector<std::string>& rsid = t.cols[0].s;                 // add_ident_columns: rsid chr bp a1 a2
    const std::vector<int32_t>& bp = t.cols[2].i;
    std::vector<double> cm(n * 4, 0.0);                                 // column-major [n x 4]: index row, size, first bp, last bp
    for (size_t i = 0; i < M; i++) {
        const int o = owner[i];
        const int k = o >= 0 ? rank[(size_t)o] : 0;
        zc.d.push_back(z[i]); pval.d.push_back(2 * pnorm_upper(fabs(z[i])));
        clump.i.push_back(k); lead.s.emplace_back(o >= 0 ? rsid[(size_t)o] : "."); rc.d.push_back(r2[i]);
        if (k < 1 || (size_t)k > n) continue;
        const size_t c = (size_t)k - 1;
        cm[c] = (double)o;
        if (cm[n + c] == 0.0) cm[2 * n + c] = (double)bp[i];            // rows come in bp order: the first member seen is the first
        cm[n + c] += 1.0;
        cm[3 * n + c] = (double)bp[i];
    }
    t.put_named("clumps", (int)n, 4, std::move(cm));
}

// P(sum lambda_i chi2_1 > q): the exact normal tail for one lambda, else Kuonen's saddlepoint approximation (Biometrika 86, 1999), with
// the one-term Edgeworth tail where the saddlepoint formula is 0 / 0 (q at the mean).  tests/sumchi2_ref.py holds the same steps.
constexpr int SUMCHI2_BISECT = 100;         // halvings of the bracket of the saddlepoint
constexpr double SUMCHI2_EDGE = 1e-3;       // |x| below which the Edgeworth tail stands in
double sumchi2_pval(const double* lam, int n, double q, int* n_pos)
{
    std::vector<double> l;
    for (int i = 0; i < n; i++) if (lam[i] > 0.0) l.push_back(lam[i]);              // (a NaN compares false)
    const int k = (int)l.size();
    if (n_pos) *n_pos = k;
    if (k == 0 || std::isnan(q)) return NAN;
    if (q <= 0.0) return 1.0;
    if (k == 1) return 2 * pnorm_upper(sqrt(q / l[0]));
    double s1 = 0, s2 = 0, s3 = 0, lmax = 0;
    for (double v : l) { s1 += v; s2 += v * v; s3 += v * v * v; lmax = std::max(lmax, v); }
    const double x = (q - s1) / sqrt(2 * s2);
    if (fabs(x) < SUMCHI2_EDGE) {
        const double k3 = 8 * s3 / ((2 * s2) * sqrt(2 * s2));
        return pnorm_upper(x) + exp(-0.5 * x * x) / 2.5066282746310002 * (k3 / 6) * (x * x - 1);
    }
    // K'(zeta) = sum lambda / (1 - 2 zeta lambda) rises from 0 (zeta -> -inf) through sum lambda (zeta = 0) to +inf (zeta -> 1 / (2 lmax));
    // below the mean K'(-k / (2 q)) < q, because every term is below 1 / (2 |zeta|)
    double lo = q > s1 ? 0.0 : -0.5 * k / q, hi = q > s1 ? 0.5 / lmax : 0.0;
    for (int it = 0; it < SUMCHI2_BISECT; it++) {
        const double mid = 0.5 * (lo + hi);
        double k1 = 0;
        for (double v : l) k1 += v / (1 - 2 * mid * v);
        if (k1 > q || !(1 - 2 * mid * lmax > 0)) hi = mid; else lo = mid;
    }
    const double zeta = 0.5 * (lo + hi);
    double K = 0, K2 = 0;
    for (double v : l) { const double d = 1 - 2 * zeta * v; K += log1p(-2 * zeta * v); K2 += 2 * v * v / (d * d); }
    K *= -0.5;
    const double w = (zeta < 0 ? -1.0 : 1.0) * sqrt(2 * (zeta * q - K)), v = zeta * sqrt(K2);
    const double p = pnorm_upper(w + log(v / w) / w);
    return std::isfinite(p) ? p : NAN;
}

gauss_table* sumchi2_output(const std::vector<std::string>& geneid, const std::vector<int32_t>& gene_off, const std::vector<std::string>& rsid,
                            const std::vector<double>& z, const int32_t* n_kept, const double* lam, const double* q, const int32_t* top,
                            const int32_t* status)
{
    const size_t ng = geneid.size(), K = GAUSS_SUMCHI2_MAX_KEPT;
    std::unique_ptr<gauss_table> t(new gauss_table());
    t->widen(11);
    Column &gid = t->add("geneid", GAUSS_COL_STR), &ns = t->add("num_snp", GAUSS_COL_INT), &nk = t->add("num_kept", GAUSS_COL_INT);
    Column &cq = t->add("chisq", GAUSS_COL_DBL), &pv = t->add("pval", GAUSS_COL_DBL), &lm = t->add("lam_max", GAUSS_COL_DBL);
    Column &np = t->add("n_pos", GAUSS_COL_INT), &st = t->add("status", GAUSS_COL_INT), &ts = t->add("top_snp", GAUSS_COL_STR);
    Column &tp = t->add("top_snp_pval", GAUSS_COL_DBL), &msg = t->add("message", GAUSS_COL_STR);
    std::vector<double> cm(ng * K, NAN);                                // column-major [ng x 128]
    for (size_t g = 0; g < ng; g++) {
        const int r0 = gene_off[g], n = gene_off[g + 1] - r0;
        const double* l = lam + g * K;
        for (size_t c = 0; c < K; c++) cm[c * ng + g] = l[c];
        int pos = 0;
        const bool solved = status[g] == 0;
        const double p = solved ? sumchi2_pval(l, (int)K, q[g], &pos) : NAN;
        gid.s.push_back(geneid[g]); ns.i.push_back(n); nk.i.push_back(n_kept[g]); cq.d.push_back(q[g]); pv.d.push_back(p);
        lm.d.push_back(solved ? l[0] : NAN); np.i.push_back(pos); st.i.push_back(status[g]);
        const int tr = top[g];
        const bool has = tr >= 0 && tr < n;
        ts.s.emplace_back(has ? rsid[(size_t)(r0 + tr)] : ".");
        tp.d.push_back(has ? 2 * pnorm_upper(fabs(z[(size_t)(r0 + tr)])) : NAN);
        char why[160] = "";
        if (status[g] & GAUSS_ST_SUMCHI2_TOOLARGE)
            snprintf(why, sizeof why, "%d SNPs survive the pruning; the eigenvalue solve takes at most %d (prune harder)", n_kept[g], GAUSS_SUMCHI2_MAX_KEPT);
        else if (status[g] & GAUSS_ST_SUMCHI2_EMPTY) snprintf(why, sizeof why, "no SNP of the gene is kept");
        else if (status[g] & GAUSS_ST_NOCONV) snprintf(why, sizeof why, "the eigenvalue solve did not converge");
        msg.s.emplace_back(why);
    }
    t->put_named("lam", (int)ng, (int)K, std::move(cm));
    return t.release();
}

int ldsplit_params(double thr_r2, int min_size, int max_size, int max_K, double max_r2, double kb, LdSplitParams& out)
{
    out.thr_r2 = std::isnan(thr_r2) ? 0.02 : thr_r2;
    out.max_r2 = std::isnan(max_r2) ? 0.3 : max_r2;
    out.min_size = min_size == 0 ? 50 : min_size;
    out.max_size = max_size == 0 ? 1000 : max_size;
    out.max_K = max_K == 0 ? GAUSS_LDSPLIT_MAX_K : max_K;
    if (!(out.thr_r2 >= 0.0 && out.thr_r2 <= 1.0)) return herr("ldsplit: thr_r2 = %g is outside [0, 1]", out.thr_r2);
    if (!(out.max_r2 >= 0.0 && out.max_r2 <= 1.0)) return herr("ldsplit: max_r2 = %g is outside [0, 1]", out.max_r2);
    if (out.max_size < 1 || out.max_size > GAUSS_LDSPLIT_MAX_SIZE)
        return herr("ldsplit: max_size = %d; a block holds 1 .. %d SNPs", out.max_size, GAUSS_LDSPLIT_MAX_SIZE);
    if (out.min_size < 1 || out.min_size > out.max_size)
        return herr("ldsplit: min_size = %d is outside 1 .. max_size = %d", out.min_size, out.max_size);
    if (out.max_K < 1 || out.max_K > GAUSS_LDSPLIT_MAX_K)
        return herr("ldsplit: max_K = %d; a call splits into 1 .. %d blocks", out.max_K, GAUSS_LDSPLIT_MAX_K);
    out.radius = (int64_t)1 << 32;                                      // no limit: positions are 32-bit
    if (!std::isnan(kb)) {
        if (!(kb >= 0.0) || !std::isfinite(kb) || kb * 1000.0 > 4e9) return herr("ldsplit: kb = %g; the distance is 0 .. 4 000 000 kb", kb);
        out.radius = (int64_t)llround(kb * 1000.0);
    }
    return 0;
}

void ldsplit_output(gauss_table& t, int M, int max_K, const double* cost, const int32_t* prev, const double* mx, int64_t n_nonfinite)
{
    const size_t Mp = (size_t)M + 1;
    std::vector<int> ks;
    for (int K = 1; K <= max_K; K++)
        if (std::isfinite(cost[K - 1])) ks.push_back(K);
    const size_t n = ks.size(), kmax = n ? (size_t)ks.back() : 0;
    std::vector<double> sp(n * 5, 0.0), last(n * kmax, -1.0);           // column-major
    for (size_t r = 0; r < n; r++) {
        const int K = ks[r];
        double sum2 = 0.0, biggest = 0.0;
        int b = M;
        for (int k = K; k >= 1; k--) {                                  // block k is rows a .. b - 1
            const int a = prev[(size_t)(k - 1) * Mp + (size_t)b];
            const double size = (double)(b - a);
            sum2 += size * size;
            biggest = std::max(biggest, size);
            last[(size_t)(k - 1) * n + r] = (double)(b - 1);
            b = a;
        }
        sp[r] = (double)K; sp[n + r] = cost[K - 1]; sp[2 * n + r] = sum2 / ((double)M * (double)M); sp[3 * n + r] = sum2; sp[4 * n + r] = biggest;
    }
    t.put_named("splits", (int)n, 5, std::move(sp));
    t.put_named("last", (int)n, (int)kmax, std::move(last));
    t.put_named("max_r2_at", (int)Mp, 1, std::vector<double>(mx, mx + Mp));
    t.put_named("n_nonfinite", 1, 1, std::vector<double>(1, (double)n_nonfinite));
}

void hess_output(gauss_table& t, int M, int T, int k_max, const double* z, const double* lam, const double* proj, int n_pos, int sweeps,
                 int64_t n_nonfinite, int status)
{
    std::vector<double> zm((size_t)M * T), pm((size_t)T * k_max);
    for (int k = 0; k < T; k++)
        for (int i = 0; i < M; i++) zm[(size_t)k * M + i] = z[(size_t)k * M + i];            // [M x T] column-major = [T][M] row-major
    for (int k = 0; k < T; k++)
        for (int i = 0; i < k_max; i++) pm[(size_t)i * T + k] = proj[(size_t)k * k_max + i];
    t.put_named("z", M, T, std::move(zm));
    t.put_named("lam", M, 1, std::vector<double>(lam, lam + M));
    t.put_named("proj", T, k_max, std::move(pm));
    t.put_named("solve", 1, 4, std::vector<double>{(double)n_pos, (double)sweeps, (double)n_nonfinite, (double)status});
    if (status & GAUSS_ST_HESS_NOCONV) t.messages.push_back("hess: the eigen-solver ran its 30 sweeps out; the values are those of the last sweep");
}

gauss_table* qcat_output(gauss_prepared& p)     // qcat.cpp:94-131 / qcatmix.cpp:102-139
{
    const bool mix = p.kind == GAUSS_KIND_QCATMIX;
    gauss_table* t = new gauss_table();
    const std::vector<Snp*> rows = window_rows(p);
    add_ident_columns(*t, rows);
    Column &af = t->add(mix ? "af1mix" : "af1ref", GAUSS_COL_DBL), &z = t->add("z", GAUSS_COL_DBL), &qm = t->add("qcat_m", GAUSS_COL_INT);
    Column &qt = t->add("qcat_t", GAUSS_COL_DBL), &qc = t->add("qcat_chisq", GAUSS_COL_DBL), &qp = t->add("qcat_pval", GAUSS_COL_DBL);
    Column& type = t->add("type", GAUSS_COL_INT);
    for (Snp* s : rows) {
        af.d.push_back(mix ? s->af1mix : s->af1ref);
        z.d.push_back(s->z);
        qm.i.push_back(s->qcat_m); qt.d.push_back(s->qcat_t); qc.d.push_back(s->qcat_chisq);
        qp.d.push_back(pchisq_upper(s->qcat_chisq, 1));           // qcat.cpp:107
        type.i.push_back(s->type);
    }
    return t;
}

// a named matrix from ROW-major data (the window outputs' layout), transposed into NamedMat's column-major one
static void put_named_rowmajor(gauss_table* t, const char* name, int nrow, int ncol, const double* row_major)
{
    std::vector<double> d((size_t)nrow * ncol);
    for (int r = 0; r < nrow; r++)
        for (int c = 0; c < ncol; c++) d[(size_t)c * nrow + r] = row_major[(size_t)r * ncol + c];
    t->put_named(name, nrow, ncol, std::move(d));
}

gauss_table* prep_output(gauss_prepared& p)     // prep_qcat.cpp:135-204 / prep_qcatmix.cpp:262-315
{
    const bool rec = p.kind == GAUSS_KIND_PREP_RECESSIVE;
    const int M = (int)p.measured.size(), U = (int)p.unmeasured.size();
    gauss_table* t = new gauss_table();
    // prep_qcat lists the whole extended window (prep_qcat.cpp:146-155), prep_recessive_impute only the
    // prediction window (prep_qcatmix.cpp:267-276)
    const std::vector<Snp*>& rows = rec ? p.unmeasured : p.snp_vec;
    add_ident_columns(*t, rows);
    Column &af = t->add(rec ? "af1mix" : "af1ref", GAUSS_COL_DBL), &z = t->add("z", GAUSS_COL_DBL), &type = t->add("type", GAUSS_COL_INT);
    for (Snp* s : rows) {
        af.d.push_back(rec ? s->af1mix : s->af1ref);
        z.d.push_back(s->z); type.i.push_back(s->type);
    }
    put_named_rowmajor(t, rec ? "zvec" : "z_vec", M, 1, p.z1.data());
    put_named_rowmajor(t, rec ? "cormat" : "cor_mat1", M, M, p.out_b11.data());
    if (!rec) put_named_rowmajor(t, "cor_mat2", U, M, p.out_b21.data());
    else {
        put_named_rowmajor(t, "cormat_add", U, M, p.out_b21.data());
        put_named_rowmajor(t, "cormat_dom", U, M, p.out_b21.data() + (size_t)U * M);
        put_named_rowmajor(t, "cormat_rec", U, M, p.out_b21.data() + (size_t)2 * U * M);
    }
    return t;
}

extern "C" {

const char* gauss_host_last_error(void) { return g_err.c_str(); }

int gauss_table_nrow(const gauss_table* t) { return t ? t->nrow() : 0; }
int gauss_table_ncol(const gauss_table* t) { return t ? (int)t->cols.size() : 0; }
const char* gauss_table_colname(const gauss_table* t, int c) { return (t && c >= 0 && c < (int)t->cols.size()) ? t->cols[c].name.c_str() : nullptr; }
int gauss_table_coltype(const gauss_table* t, int c) { return (t && c >= 0 && c < (int)t->cols.size()) ? t->cols[c].type : -1; }
const char* gauss_table_str(const gauss_table* t, int c, int r)
{
    if (!t || c < 0 || c >= (int)t->cols.size() || t->cols[c].type != GAUSS_COL_STR || r < 0 || r >= (int)t->cols[c].s.size()) return nullptr;
    return t->cols[c].s[r].c_str();
}
const int32_t* gauss_table_int(const gauss_table* t, int c) { return (t && c >= 0 && c < (int)t->cols.size() && t->cols[c].type == GAUSS_COL_INT) ? t->cols[c].i.data() : nullptr; }
const double* gauss_table_dbl(const gauss_table* t, int c) { return (t && c >= 0 && c < (int)t->cols.size() && t->cols[c].type == GAUSS_COL_DBL) ? t->cols[c].d.data() : nullptr; }
const double* gauss_table_matrix(const gauss_table* t, int* n) { if (!t || t->matrix.empty()) { if (n) *n = 0; return nullptr; } if (n) *n = t->matrix_n; return t->matrix.data(); }
const char* gauss_table_strcol(const gauss_table* t, int c, int64_t* bytes)
{
    if (!t || c < 0 || c >= (int)t->cols.size() || t->cols[c].type != GAUSS_COL_STR) return nullptr;
    const Column& col = t->cols[c];
    if (col.joined.empty() && !col.s.empty()) {
        size_t n = 0;
        for (const std::string& v : col.s) n += v.size() + 1;
        col.joined.reserve(n);
        for (const std::string& v : col.s) { col.joined += v; col.joined.push_back('\0'); }
    }
    if (bytes) *bytes = (int64_t)col.joined.size();
    return col.joined.data();
}
void gauss_table_free(gauss_table* t) { delete t; }
int gauss_table_n_named(const gauss_table* t) { return t ? (int)t->named.size() : 0; }
const char* gauss_table_named_name(const gauss_table* t, int k) { return (t && k >= 0 && k < (int)t->named.size()) ? t->named[k].name.c_str() : nullptr; }
const double* gauss_table_named(const gauss_table* t, int k, int* nrow, int* ncol)
{
    if (!t || k < 0 || k >= (int)t->named.size()) return nullptr;
    if (nrow) *nrow = t->named[k].nrow;
    if (ncol) *ncol = t->named[k].ncol;
    return t->named[k].d.data();
}

// The JEPEG k x k tail of one gene on the host, as run_jepeg calls it after the GPU has produced CorG: exposed so that
// it can be checked on its own (no GPU involved).  corg is n x n (symmetric), has / wgt are n x 6 row-major.
int gauss_host_jepeg_gene_tail(int n, const double* corg, const double* z, const double* info, const int32_t* has,
                               const double* wgt, double* chisq, int32_t* df, double* jepeg_pval, int32_t* top_categ,
                               double* top_categ_pval, int32_t* top_snp, double* top_snp_pval)
{
    if (n < 0 || (n > 0 && (!corg || !z || !info || !has || !wgt))) return herr("bad arguments");
    Args a;
    std::vector<std::unique_ptr<Snp>> own;
    std::vector<Snp*> gs;
    for (int s = 0; s < n; s++) {
        own.emplace_back(new Snp());
        Snp& sn = *own.back();
        sn.rsid = std::to_string(s); sn.z = z[s]; sn.info = info[s]; sn.geneid = "G";
        for (int c = 0; c < 6; c++) if (has[(size_t)s * 6 + c]) sn.categ[c] = wgt[(size_t)s * 6 + c];
        gs.push_back(&sn);
    }
    const GeneResult r = jepeg_tail(gs, corg, a);
    if (chisq) *chisq = r.chisq;
    if (df) *df = r.df;
    if (jepeg_pval) *jepeg_pval = r.jepeg_pval;
    if (top_categ) { *top_categ = -1; for (int c = 0; c < 6; c++) if (r.top_categ == categ_name(c)) *top_categ = c; }
    if (top_categ_pval) *top_categ_pval = r.top_categ_pval;
    if (top_snp) *top_snp = (r.top_snp == ".") ? -1 : atoi(r.top_snp.c_str());
    if (top_snp_pval) *top_snp_pval = r.top_snp_pval;
    return 0;
}

int gauss_table_n_messages(const gauss_table* t) { return t ? (int)t->messages.size() : 0; }
const char* gauss_table_message(const gauss_table* t, int k) { return (t && k >= 0 && k < (int)t->messages.size()) ? t->messages[k].c_str() : nullptr; }

}  // extern "C"
void build_fixed_image(const Column& col)
{
    size_t w = 1;
    for (const std::string& v : col.s) w = std::max(w, v.size());
    if (col.fixed.size() == w * col.s.size() && col.fixed_w == (int)w && !col.s.empty()) return;       // made already (rows are not edited afterwards)
    col.fixed.assign(w * col.s.size(), '\0');
    for (size_t r = 0; r < col.s.size(); r++) memcpy(&col.fixed[r * w], col.s[r].data(), col.s[r].size());
    col.fixed_w = (int)w;
}
extern "C" {
// A whole string column as one fixed-width, NUL-padded byte matrix [nrow x *width] (numpy dtype "S<width>"):
// 90 000 rows come across the boundary as one buffer instead of 90 000 Python strings.
const char* gauss_table_strcol_fixed(const gauss_table* t, int c, int* width)
{
    if (!t || c < 0 || c >= (int)t->cols.size() || t->cols[c].type != GAUSS_COL_STR) return nullptr;
    const Column& col = t->cols[c];
    build_fixed_image(col);
    if (width) *width = col.fixed_w;
    return col.fixed.data();
}

}  // extern "C"
