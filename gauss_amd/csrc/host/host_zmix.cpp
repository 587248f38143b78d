// libgauss_host.so -- zmix() (zmix.R): ancestry proportions of a study from its Z-scores.  The SNP selection is prep_zmix5's
// (host_calls.cpp: zmix_read / zmix_ai_select); the normal equations X^T X, X^T y of the pair matrix that prep_zmix5 /
// prep_zmix5_sup would return are reduced on the GPU (gauss_zmix_normal_eq) without forming that matrix; the host then solves
// quadprog::solve.QP's problem -- min 1/2 w^T D w - d^T w subject to sum w = 1, w >= 0, -w >= -1 -- by the Goldfarb-Idnani dual
// active-set method that solve.QP implements, normalises, rounds to 5 decimals and normalises again (zmix.R).
#include "host_internal.h"

#include <cfloat>
#include <fstream>

namespace {

// Goldfarb & Idnani (1983), "A numerically stable dual method for solving strictly convex quadratic programs", as quadprog's
// qpgen2 implements it: min 1/2 x^T D x - d^T x subject to N^T x >= b, the first meq constraints equalities.  The dense
// constraint matrix N is n x m, column-major.  J = L^-T Q and the upper-triangular R with J^T N_A = [R; 0] are kept and updated
// by Givens rotations as constraints enter and leave the active set A.  Returns 0, or -1 with the error set.
int solve_qp_gi(const std::vector<double>& D, const std::vector<double>& dvec, int n, const std::vector<double>& N,
                const std::vector<double>& b, int meq, std::vector<double>& x)
{
    const int m = (int)b.size();
    auto col = [&](int i) { return &N[(size_t)i * n]; };
    // Cholesky D = L L^T (lower L, row-major); a pivot <= 0 is quadprog's error.  A pivot within rounding of 0 (n eps D_jj) counts
    // as 0: D with two equal columns leaves s - (s / sqrt(s))^2, which rounds to 0 or to either side of it
    std::vector<double> L((size_t)n * n, 0.0);
    for (int j = 0; j < n; j++) {
        double s = D[(size_t)j * n + j];
        for (int k = 0; k < j; k++) s -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(s > n * DBL_EPSILON * D[(size_t)j * n + j])) return herr("matrix D in quadratic function is not positive definite!");
        const double ljj = std::sqrt(s);
        L[(size_t)j * n + j] = ljj;
        for (int i = j + 1; i < n; i++) {
            double t = D[(size_t)i * n + j];
            for (int k = 0; k < j; k++) t -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = t / ljj;
        }
    }
    // J = L^-T (J[r][c] row-major: column c of J is J[. * n + c]); x = D^-1 d, the unconstrained minimum
    std::vector<double> J((size_t)n * n, 0.0);
    for (int c = 0; c < n; c++) {                        // column c of L^-1 by forward substitution -> row c of J
        std::vector<double> e((size_t)n, 0.0);
        e[(size_t)c] = 1.0;
        for (int i = 0; i < n; i++) {
            double s = e[(size_t)i];
            for (int k = 0; k < i; k++) s -= L[(size_t)i * n + k] * e[(size_t)k];
            e[(size_t)i] = s / L[(size_t)i * n + i];
        }
        for (int i = 0; i < n; i++) J[(size_t)c * n + i] = e[(size_t)i];     // J = (L^-1)^T
    }
    x.assign((size_t)n, 0.0);
    for (int i = 0; i < n; i++) {                        // x = J J^T d
        double s = 0.0;
        for (int k = 0; k < n; k++) s += J[(size_t)k * n + i] * dvec[(size_t)k];
        for (int r = 0; r < n; r++) x[(size_t)r] += J[(size_t)r * n + i] * s;
    }
    std::vector<double> nrm((size_t)m);
    for (int i = 0; i < m; i++) {
        double s = 0.0;
        for (int k = 0; k < n; k++) s += col(i)[k] * col(i)[k];
        nrm[(size_t)i] = std::sqrt(s);
    }
    std::vector<double> R((size_t)n * n, 0.0);          // R[r * n + c], upper triangular, q x q used
    std::vector<int> act;                                // active constraints, in R's column order
    std::vector<double> u;                               // their multipliers
    std::vector<char> is_act((size_t)m, 0);
    std::vector<double> dd((size_t)n), z((size_t)n), r((size_t)n), np((size_t)n);
    auto rotate_cols = [&](int a, int c2, double cs, double sn) {   // J[:, a], J[:, c2] <- (c J_a + s J_c2, -s J_a + c J_c2)
        for (int k = 0; k < n; k++) {
            const double ja = J[(size_t)k * n + a], jb = J[(size_t)k * n + c2];
            J[(size_t)k * n + a] = cs * ja + sn * jb;
            J[(size_t)k * n + c2] = -sn * ja + cs * jb;
        }
    };
    const int max_iter = 50 * (m + n) + 100;
    for (int iter = 0;; iter++) {
        if (iter > max_iter) return herr("zmix: the quadratic program did not converge in %d steps", max_iter);
        // ---- the most violated constraint, each scaled by its norm (qpgen2); |s| below a rounding-level tolerance counts as 0
        double xn = 0.0;
        for (int k = 0; k < n; k++) xn = std::max(xn, std::fabs(x[(size_t)k]));
        int p = -1;
        double worst = 0.0, sp = 0.0;
        for (int i = 0; i < m; i++) {
            if (is_act[(size_t)i]) continue;
            double s = -b[(size_t)i];
            for (int k = 0; k < n; k++) s += col(i)[k] * x[(size_t)k];
            const double tol = 1e-14 * (nrm[(size_t)i] * xn + std::fabs(b[(size_t)i]) + 1e-300);
            if (std::fabs(s) <= tol) continue;
            const double v = (i < meq ? -std::fabs(s) : s) / nrm[(size_t)i];
            if (v < worst) { worst = v; p = i; sp = s; }
        }
        if (p < 0) return 0;                             // feasible: x is optimal
        const double sg = (p < meq && sp > 0) ? -1.0 : 1.0;           // an equality above its bound enters as -n^T x >= -b
        for (int k = 0; k < n; k++) np[(size_t)k] = sg * col(p)[k];
        double s_p = sg * sp;                            // < 0
        double u_new = 0.0;
        for (;;) {
            const int q = (int)act.size();
            // d = J^T n_p; z = J_2 d_2 (primal direction); r = R^-1 d_1 (the dual one)
            double dn = 0.0;
            for (int c = 0; c < n; c++) {
                double s = 0.0;
                for (int k = 0; k < n; k++) s += J[(size_t)k * n + c] * np[(size_t)k];
                dd[(size_t)c] = s;
                dn += s * s;
            }
            double ztn = 0.0;
            for (int c = q; c < n; c++) ztn += dd[(size_t)c] * dd[(size_t)c];
            for (int k = 0; k < n; k++) {
                double s = 0.0;
                for (int c = q; c < n; c++) s += J[(size_t)k * n + c] * dd[(size_t)c];
                z[(size_t)k] = s;
            }
            for (int i = q - 1; i >= 0; i--) {
                double s = dd[(size_t)i];
                for (int c = i + 1; c < q; c++) s -= R[(size_t)i * n + c] * r[(size_t)c];
                r[(size_t)i] = s / R[(size_t)i * n + i];
            }
            // partial step t1: the first active inequality whose multiplier reaches 0; full step t2: n_p^T x reaches b_p
            double t1 = INFINITY;
            int kd = -1;
            for (int j = 0; j < q; j++)
                if (act[(size_t)j] >= meq && r[(size_t)j] > 0.0) {
                    const double tj = u[(size_t)j] / r[(size_t)j];
                    if (tj < t1) { t1 = tj; kd = j; }
                }
            const bool dependent = ztn <= 1e-20 * dn;    // n_p lies in the span of the active normals: no primal step
            const double t2 = dependent ? INFINITY : -s_p / ztn;
            const double t = std::min(t1, t2);
            if (!std::isfinite(t)) return herr("constraints are inconsistent, no solution!");
            for (int j = 0; j < q; j++) u[(size_t)j] -= t * r[(size_t)j];
            u_new += t;
            if (!dependent) {
                for (int k = 0; k < n; k++) x[(size_t)k] += t * z[(size_t)k];
                s_p += t * ztn;
            }
            if (!dependent && t2 <= t1) {
                // full step: p joins the active set -- rotate d_2 into its first entry, R gains the column d_1..q
                for (int c = n - 1; c > q; c--) {
                    const double a0 = dd[(size_t)c - 1], a1 = dd[(size_t)c];
                    if (a1 == 0.0) continue;
                    const double h = std::hypot(a0, a1), cs = a0 / h, sn = a1 / h;
                    dd[(size_t)c - 1] = h; dd[(size_t)c] = 0.0;
                    rotate_cols(c - 1, c, cs, sn);
                }
                for (int i = 0; i <= q; i++) R[(size_t)i * n + q] = dd[(size_t)i];
                act.push_back(p); u.push_back(u_new);
                is_act[(size_t)p] = 1;
                break;
            }
            // partial step: constraint kd leaves; R loses column kd and is brought back to upper-triangular form
            is_act[(size_t)act[(size_t)kd]] = 0;
            for (int c = kd; c < q - 1; c++)
                for (int i = 0; i < n; i++) R[(size_t)i * n + c] = R[(size_t)i * n + c + 1];
            for (int i = 0; i < n; i++) R[(size_t)i * n + q - 1] = 0.0;
            act.erase(act.begin() + kd); u.erase(u.begin() + kd);
            for (int j = kd; j < q - 1; j++) {
                const double a0 = R[(size_t)j * n + j], a1 = R[(size_t)(j + 1) * n + j];
                if (a1 == 0.0) continue;
                const double h = std::hypot(a0, a1), cs = a0 / h, sn = a1 / h;
                for (int c = j; c < q - 1; c++) {
                    const double ra = R[(size_t)j * n + c], rb = R[(size_t)(j + 1) * n + c];
                    R[(size_t)j * n + c] = cs * ra + sn * rb;
                    R[(size_t)(j + 1) * n + c] = -sn * ra + cs * rb;
                }
                R[(size_t)(j + 1) * n + j] = 0.0;
                rotate_cols(j, j + 1, cs, sn);
            }
        }
    }
}

// R's sum() of doubles accumulates in long double (summary.c rsum); so does this
double r_sum(const std::vector<double>& v)
{
    long double s = 0.0L;
    for (double x : v) s += x;
    return (double)s;
}

int zmix_qp(const double* D, const double* d, int P, double* w_unrounded, double* w_final)
{
    if (!D || !d || P < 1) return herr("bad arguments to gauss_host_zmix_qp");
    // zmix.R: Amat = cbind(rep(1, P), diag(P), -diag(P)), bvec = c(1, rep(0, P), rep(-1, P)), meq = 1
    const int m = 1 + 2 * P;
    std::vector<double> N((size_t)m * P, 0.0), b((size_t)m, 0.0);
    for (int k = 0; k < P; k++) N[(size_t)k] = 1.0;
    b[0] = 1.0;
    for (int k = 0; k < P; k++) {
        N[(size_t)(1 + k) * P + k] = 1.0;
        N[(size_t)(1 + P + k) * P + k] = -1.0;
        b[(size_t)(1 + P + k)] = -1.0;
    }
    std::vector<double> Dm(D, D + (size_t)P * P), dv(d, d + P), w;
    if (solve_qp_gi(Dm, dv, P, N, b, 1, w)) return -1;
    // weights / sum(weights); round(weights, 5); weights / sum(weights).  R >= 4.0.0's round(x, 5) picks the closer of the two
    // 5-decimal candidates around x (long-double arithmetic, ties by the shorter decimal representation); round-half-even of
    // x * 1e5 agrees with it except when x lies within about one ulp of a half-way point xxxxx.5e-5
    double s = r_sum(w);
    for (double& v : w) v = v / s;
    if (w_unrounded) for (int k = 0; k < P; k++) w_unrounded[k] = w[(size_t)k];
    for (double& v : w) v = std::nearbyint(v * 1e5) / 1e5;
    s = r_sum(w);
    for (double& v : w) v = v / s;
    if (w_final) for (int k = 0; k < P; k++) w_final[k] = w[(size_t)k];
    return 0;
}

// The description file's Population_Abbreviation and Super_Population columns, found by name in the header as zmix.R's
// read.table(header = TRUE) finds them.  Fields are split on tabs and spaces alike: the panels' description files are
// tab-separated, and read_ref_desc (which the rest of the pipeline uses) splits on either.
int read_desc_columns(const std::string& path, std::vector<std::string>& pops, std::vector<std::string>& sups)
{
    std::ifstream in(path.c_str());
    if (!in) return herr("ERROR: can't open reference population description file '%s'", path.c_str());
    auto split = [](const std::string& line) {
        std::vector<std::string> f;
        std::string tok;
        for (char c : line) {
            if (c == '\t' || c == ' ' || c == '\r') { if (!tok.empty()) f.push_back(tok); tok.clear(); }
            else tok.push_back(c);
        }
        if (!tok.empty()) f.push_back(tok);
        return f;
    };
    std::string line;
    if (!std::getline(in, line)) line.clear();
    const std::vector<std::string> head = split(line);
    int ip = -1, is = -1;
    for (int k = 0; k < (int)head.size(); k++) {
        if (head[(size_t)k] == "Population_Abbreviation" && ip < 0) ip = k;
        if (head[(size_t)k] == "Super_Population" && is < 0) is = k;
    }
    if (ip < 0 || is < 0) return herr("zmix: reference_pop_desc_file must include Population_Abbreviation and Super_Population columns.");
    while (std::getline(in, line)) {
        const std::vector<std::string> f = split(line);
        if (f.empty()) continue;                                                 // blank.lines.skip
        pops.push_back(ip < (int)f.size() ? f[(size_t)ip] : "");
        sups.push_back(is < (int)f.size() ? f[(size_t)is] : "");
    }
    return 0;
}

}  // namespace

extern "C" {

int gauss_host_zmix_qp(const double* D, const double* d, int P, double* w_unrounded, double* w_final)
{
    return zmix_qp(D, d, P, w_unrounded, w_final);
}

int gauss_host_zmix(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                    const char* reference_pop_desc_file, double percentile, int interval, int level, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    *out = nullptr;
    if (files_ok({input_file, reference_index_file, reference_data_file, reference_pop_desc_file})) return -1;
    if (level != GAUSS_ZMIX_POPULATION && level != GAUSS_ZMIX_SUPERPOPULATION)
        return herr("zmix: level %d is neither GAUSS_ZMIX_POPULATION nor GAUSS_ZMIX_SUPERPOPULATION", level);
    const bool sup = level == GAUSS_ZMIX_SUPERPOPULATION;
    const double pct = std::isnan(percentile) ? 0.9 : percentile;              // zmix.R's defaults, not prep_zmix5's
    const int step = interval > 0 ? interval : 10;
    ZmixStudy st;
    if (zmix_read(st, input_file, reference_index_file, reference_data_file, reference_pop_desc_file)) return -1;
    Args& a = st.a;
    std::vector<int> kept;
    std::vector<double> kept_nv;
    std::vector<Snp*> sel;
    if (zmix_ai_select(st, step, pct, kept, kept_nv, &sel)) return -1;
    const int S = (int)sel.size(), P = a.num_pops;
    std::vector<int32_t> pop_group;
    std::vector<std::string> group_names;
    const int G = sup ? zmix_sup_groups(a, pop_group, group_names) : P;
    if (G > 64) return herr("zmix: %d %s; the normal equations hold 1 .. 64", G, sup ? "super-populations" : "populations");
    if (S < 2) return herr("zmix: no valid rows after filtering.");            // no pairs at all
    int N = 0;
    const std::vector<int32_t> pop_off = panel_pop_off(a, &N);
    int64_t ld = 0;
    std::vector<uint8_t> geno;
    if (zmix_genotypes(a, sel, N, &ld, geno)) return -1;
    std::vector<double> z((size_t)S);
    for (int i = 0; i < S; i++) z[(size_t)i] = sel[(size_t)i]->z;
    std::vector<double> xtx((size_t)G * G), xty((size_t)G);
    double yty = 0.0;
    int64_t n_rows = 0;
    if (gauss_zmix_normal_eq(ctx, geno.data(), S, ld, pop_off.data(), P, sup ? pop_group.data() : nullptr, G, z.data(), xtx.data(),
                             xty.data(), &yty, &n_rows) != GAUSS_OK)
        return herr("%s", gauss_last_error());
    if (n_rows == 0) return herr("zmix: no valid rows after filtering.");
    std::vector<std::string> pops, sups;
    if (read_desc_columns(a.reference_pop_desc_file, pops, sups)) return -1;
    std::vector<std::string> names;
    if (sup) {
        for (const std::string& s : sups)
            if (std::find(names.begin(), names.end(), s) == names.end()) names.push_back(s);
        if ((int)names.size() != G) return herr("zmix: column count mismatch between prep_zmix5_sup output and superpopulation metadata.");
    } else if ((int)pops.size() != G) {
        return herr("zmix: column count mismatch between prep_zmix5 output and population metadata.");
    }
    std::vector<double> w_unr((size_t)G), w((size_t)G);
    if (zmix_qp(xtx.data(), xty.data(), G, w_unr.data(), w.data())) return -1;
    std::unique_ptr<gauss_table> t(new gauss_table());
    if (sup) {
        t->add("SuperPopulation", GAUSS_COL_STR).s = names;
    } else {
        t->add("Population", GAUSS_COL_STR).s = pops;
        t->add("SuperPopulation", GAUSS_COL_STR).s = sups;
    }
    t->add("Weight", GAUSS_COL_DBL).d = w;
    t->put_named("dmat", G, G, xtx);                    // symmetric: row- and column-major agree
    t->put_named("dvec", G, 1, xty);
    t->put_named("w_unrounded", G, 1, w_unr);
    t->put_named("n_snp", 1, 1, {(double)S});
    t->put_named("n_pairs", 1, 1, {(double)S * (double)(S - 1) / 2});
    t->put_named("n_rows", 1, 1, {(double)n_rows});
    t->put_named("yty", 1, 1, {yty});
    *out = t.release();
    return 0;
}

}  // extern "C"
