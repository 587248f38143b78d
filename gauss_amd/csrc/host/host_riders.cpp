// libgauss_host.so -- the riders of a one-window call (host_internal.h: Rider): what dist() / distmix() are asked beyond the plain
// table.  Each rides in the window's single job through its own fields of gauss_window_desc and builds its table from the
// WindowView of the call, whichever way the window was built.
#include "host_internal.h"

// ---- loo ----
int LooRider::ask(gauss_window_desc& d, const WindowView&)
{
    z.assign((size_t)d.n_measured, 0.0); info = z; t = z;
    d.out_loo_z = z.data(); d.out_loo_info = info.data(); d.out_loo_t = t.data();
    return 0;
}

int LooRider::table(const WindowView& v, gauss_table** out)
{
    std::vector<LooRow> rows;
    for (size_t i = 0; i < v.measured.size(); i++) {
        const ViewSnp& s = v.measured[i];
        if (!s.wing) rows.push_back(LooRow{s.id, s.af, s.z, (int)i});
    }
    *out = loo_output(v.mix, rows, z.data(), info.data(), t.data());
    return 0;
}

// ---- slct, cond ----
int SlctRider::ask(gauss_window_desc& d, const WindowView& v)
{
    const int K = max_signals <= 0 ? GAUSS_SLCT_MAX : max_signals;
    const double r2 = collin <= 0 ? 0.9 : collin;
    if (K > GAUSS_SLCT_MAX) return herr("max_signals = %d: at most %d signals are selected", K, GAUSS_SLCT_MAX);
    if (n_cond < 0 || (n_cond > 0 && !cond)) return herr("bad cond_rsids");
    if (n_cond > K) return herr("%d conditioning SNPs, but max_signals = %d", n_cond, K);
    for (int c = 0; c < n_cond; c++) {
        int at = -1;
        for (size_t i = 0; i < v.measured.size() && at < 0; i++)
            if (cond[c] && !strcmp(cond[c], v.measured[i].id.rsid)) at = (int)i;
        if (at < 0) return herr("cond_rsids: %s is not a measured SNP of the extended window", cond[c] ? cond[c] : "(null)");
        for (int32_t f : forced) if (f == at) return herr("cond_rsids: %s is listed twice", cond[c]);
        forced.push_back(at);
    }
    idx.assign((size_t)K, -1); zin.assign((size_t)K, NAN); joint = zin;
    zc.assign((size_t)d.n_measured, NAN); var = zc;
    d.slct_max = K;
    d.slct_chi2_stop = slct_chi2_of(p_cutoff <= 0 ? 5e-8 : p_cutoff);
    d.slct_min_var_frac = 1.0 - r2 / ((1.0 + d.lambda) * (1.0 + d.lambda));      // "un-ridged r^2 >= collin" (include/gauss_hip.h)
    d.slct_forced = forced.empty() ? nullptr : forced.data(); d.n_slct_forced = (int)forced.size();
    d.out_slct_n = &n; d.out_slct_idx = idx.data(); d.out_slct_zin = zin.data(); d.out_slct_joint = joint.data();
    d.out_slct_zc = zc.data(); d.out_slct_var = var.data();
    if (unmeasured) {
        // the ridge does not cap what the signals explain of an imputed SNP, so "r^2 >= collin" is 1 - collin here, without the
        // (1 + lambda)^2 of the measured SNPs' guard (include/gauss_hip.h)
        cond_z.assign((size_t)std::max(d.n_unmeasured, 1), NAN); cond_var = cond_z;
        d.cond_min_var_frac = 1.0 - r2;
        d.out_cond_z = cond_z.data(); d.out_cond_var = cond_var.data();
    }
    return 0;
}

int SlctRider::table(const WindowView& v, gauss_table** out)
{
    if (!unmeasured) {
        *out = slct_output(v.mix, v.measured, n, idx.data(), zin.data(), joint.data(), zc.data(), var.data());
        return 0;
    }
    if (v.plain(out)) return -1;
    if (cond_output(**out, v.measured, v.row_m, v.row_u, n, idx.data(), zin.data(), joint.data(), zc.data(), var.data(), cond_z.data(), cond_var.data())) {
        gauss_table_free(*out); *out = nullptr;
        return -1;
    }
    return 0;
}

// ---- cs ----
int CsRider::ask(gauss_window_desc& d, const WindowView& v)
{
    if (SlctRider::ask(d, v)) return -1;
    const size_t T = (size_t)std::max(d.n_measured + d.n_unmeasured, 1), K = (size_t)d.slct_max;
    pip.assign(T, NAN); set_pip = pip; set.assign(T, -1);
    size.assign(K, 0); mass.assign(K, NAN); lse = mass;
    d.cs_coverage = coverage > 0 ? coverage : 0.95;                    // (a NaN compares false: the default)
    d.cs_prior_var = prior_var > 0 ? prior_var : 25.0;                 // a prior s.d. of 5 on the non-centrality: this project's default
    d.out_cs_pip = pip.data(); d.out_cs_set = set.data(); d.out_cs_set_pip = set_pip.data();
    d.out_cs_size = size.data(); d.out_cs_mass = mass.data(); d.out_cs_lse = lse.data();
    return 0;
}

int CsRider::table(const WindowView& v, gauss_table** out)
{
    if (SlctRider::table(v, out)) return -1;
    if (cs_output(**out, v.measured, v.row_m, v.row_u, n, idx.data(), pip.data(), set.data(), set_pip.data(), size.data(), mass.data(), lse.data())) {
        gauss_table_free(*out); *out = nullptr;
        return -1;
    }
    return 0;
}

// ---- susie ----
int SusieRider::check()
{
    if (L > GAUSS_SUSIE_MAX_L) return herr("L = %d: the multi-causal fit takes at most %d effects", L, GAUSS_SUSIE_MAX_L);
    return 0;
}

int SusieRider::ask(gauss_window_desc& d, const WindowView&)
{
    n_eff = L > 0 ? L : 10;
    const size_t T = (size_t)std::max(d.n_measured + d.n_unmeasured, 1), K = (size_t)n_eff;
    pip.assign(T, NAN); set_pip = pip; set.assign(T, -1); alpha.assign(K * T, NAN);
    V.assign(K, NAN); lse = V; mass = V; purity = V; size.assign(K, 0); kept = size; sweeps.assign(2, NAN); sweeps[0] = 0.0;
    tol_used = tol < 0 ? 0.0 : (tol > 0 ? tol : 1e-4);                 // negative: exactly max_sweeps sweeps; 0 or NaN: the default
    d.susie_L = n_eff;
    d.susie_coverage = coverage > 0 ? coverage : 0.95;                 // (a NaN compares false: the default)
    d.susie_prior_var = prior_var > 0 ? prior_var : 25.0;              // a prior s.d. of 5 on an effect, in z units: this project's default, as for *_cs
    d.susie_min_abs_corr = min_abs_corr > 0 ? min_abs_corr : 0.5;
    d.susie_max_sweeps = max_sweeps > 0 ? max_sweeps : 100;
    d.susie_tol = tol_used;
    d.susie_estimate_var = estimate_prior_var < 0 ? 1 : (estimate_prior_var ? 1 : 0);      // negative: the default, on
    d.susie_measured_only = measured_only > 0 ? 1 : 0;
    d.out_susie_pip = pip.data(); d.out_susie_set = set.data(); d.out_susie_set_pip = set_pip.data(); d.out_susie_alpha = alpha.data();
    d.out_susie_V = V.data(); d.out_susie_lse = lse.data(); d.out_susie_mass = mass.data(); d.out_susie_purity = purity.data();
    d.out_susie_size = size.data(); d.out_susie_kept = kept.data(); d.out_susie_sweeps = sweeps.data();
    return 0;
}

int SusieRider::table(const WindowView& v, gauss_table** out)
{
    if (v.plain(out)) return -1;
    if (susie_output(**out, v.measured, v.row_m, v.row_u, n_eff, tol_used, pip.data(), set.data(), set_pip.data(), alpha.data(), V.data(), lse.data(),
                     size.data(), mass.data(), purity.data(), kept.data(), sweeps.data())) {
        gauss_table_free(*out); *out = nullptr;
        return -1;
    }
    return 0;
}

// ---- prs ----
// lassosum's grid: s = 0.2, 0.5, 0.9, 1 and 20 penalties log-spaced from 0.1 down to 0.001
PrsRider::PrsRider(double n_, const double* s_, int n_s, const double* lam_, int n_lam, double tol_, int max_sweeps_)
    : n(n_), tol(tol_), max_sweeps(max_sweeps_), n_s_arg(n_s), n_lam_arg(n_lam)
{
    if (s_ && n_s > 0) s.assign(s_, s_ + n_s);
    else s = {0.2, 0.5, 0.9, 1.0};
    if (lam_ && n_lam > 0) lam.assign(lam_, lam_ + n_lam);
    else
        for (int k = 0; k < 20; k++) lam.push_back(exp(log(0.1) + (log(0.001) - log(0.1)) * k / 19.0));
}

int PrsRider::check()
{
    if (n_s_arg > GAUSS_PRS_MAX_S) return herr("%d shrinkage values: the score takes at most %d", n_s_arg, GAUSS_PRS_MAX_S);
    if (n_lam_arg > GAUSS_PRS_MAX_LAM) return herr("%d penalties: the score takes at most %d", n_lam_arg, GAUSS_PRS_MAX_LAM);
    return 0;
}

int PrsRider::ask(gauss_window_desc& d, const WindowView&)
{
    const size_t M = (size_t)std::max(d.n_measured, 1), nc = s.size() * lam.size();
    beta.assign(nc * M, NAN); delta.assign(nc, NAN); br = delta; bg = delta; kkt = delta;
    nnz.assign(nc, 0); sweeps = nnz;
    tol_used = tol != 0 && tol == tol ? tol : 1e-4;                    // 0 or NaN: the default; a negative one is the window's to refuse
    d.prs_n_s = (int)s.size(); d.prs_n_lam = (int)lam.size(); d.prs_s = s.data(); d.prs_lam = lam.data();
    d.prs_n = n; d.prs_tol = tol_used; d.prs_max_sweeps = max_sweeps > 0 ? max_sweeps : 100;
    d.out_prs_beta = beta.data(); d.out_prs_nnz = nnz.data(); d.out_prs_sweeps = sweeps.data(); d.out_prs_delta = delta.data();
    d.out_prs_br = br.data(); d.out_prs_bg = bg.data(); d.out_prs_kkt = kkt.data();
    return 0;
}

int PrsRider::table(const WindowView& v, gauss_table** out)
{
    *out = prs_output(v.mix, v.measured, n, tol_used, s, lam, beta.data(), nnz.data(), sweeps.data(), delta.data(), br.data(), bg.data(), kkt.data());
    return 0;
}

// ---- traits, traits_miss ----
int TraitsRider::check()
{
    if (n_more < 0 || (n_more > 0 && !files)) return herr("bad more_input_files");
    if (n_more > GAUSS_TRAITS_MORE_MAX) return herr("%d further traits: a call takes at most %d", n_more, GAUSS_TRAITS_MORE_MAX);
    for (int k = 0; k < n_more; k++) if (files_ok({files[k]})) return -1;
    return 0;
}

int TraitsRider::ask(gauss_window_desc& d, const WindowView& v)
{
    const size_t M = (size_t)d.n_measured, U = (size_t)d.n_unmeasured;
    z.assign((size_t)n_more * M, 0.0); out_z.assign((size_t)n_more * U, 0.0);
    if (miss) mask.assign((size_t)n_more * M, 0);
    size_t n_miss = 0;
    for (int k = 0; k < n_more; k++) {
        std::string err;
        std::shared_ptr<const GwasCache> gw = load_gwas_cached(files[k], err);
        if (!gw) return herr("%s", err.c_str());
        size_t lacks = 0;
        if (traits_match(*gw, files[k], M, [&](size_t i) { return v.measured[i].id; }, z.data() + (size_t)k * M,
                         miss ? mask.data() + (size_t)k * M : nullptr, &lacks)) return -1;
        n_miss += lacks;
    }
    if (n_more > 0) { d.n_traits_more = n_more; d.z_more = z.data(); d.out_z_more = out_z.data(); }
    if (n_more > 0 && miss) {
        if (traits_miss_limits(files, n_more, M, mask.data(), Args().min_num_measured_snp)) return -1;
        info.assign((size_t)n_more * U, 0.0); z_miss.assign(std::max<size_t>(n_miss, 1), 0.0); info_miss = z_miss;
        d.miss_more = mask.data(); d.out_info_more = info.data(); d.out_z_miss = z_miss.data(); d.out_info_miss = info_miss.data();
    }
    return 0;
}

int TraitsRider::table(const WindowView& v, gauss_table** out)
{
    if (v.plain(out)) return -1;
    const TraitsMiss tm = {mask.data(), info.data(), z_miss.data(), info_miss.data()};
    traits_output(**out, n_more, v.row_m, v.row_u, z.data(), out_z.data(), n_more > 0 && miss ? &tm : nullptr);
    return 0;
}

// ---- coloc ----
int ColocRider::check()
{
    if (traits.check() || susie.check()) return -1;
    if (traits.n_more < 1) return herr("the colocalisation takes at least two study files (the first is trait 1)");
    if (traits.n_more > GAUSS_SUSIE_TRAITS_MORE_MAX)
        return herr("%d study files: at most %d traits are fitted in one window", 1 + traits.n_more, 1 + GAUSS_SUSIE_TRAITS_MORE_MAX);
    return 0;
}

int ColocRider::ask(gauss_window_desc& d, const WindowView& v)
{
    if (traits.ask(d, v) || susie.ask(d, v)) return -1;
    const size_t k = (size_t)traits.n_more, L = (size_t)susie.n_eff, T = (size_t)std::max(d.n_measured + d.n_unmeasured, 1);
    const size_t np = (k + 1) * k / 2;
    pip.assign(k * T, NAN); set_pip = pip; set.assign(k * T, -1); alpha.assign(k * L * T, NAN);
    V.assign(k * L, NAN); lse = V; mass = V; purity = V; size.assign(k * L, 0); kept = size; sweeps.assign(2 * k, NAN);
    for (size_t t = 0; t < k; t++) sweeps[2 * t] = 0.0;
    pp.assign(5 * np * L * L, NAN); hit_pp.assign(np * L * L, NAN); hit.assign(np * L * L, -1); n.assign(np, 0);
    d.coloc_traits_more = (int)k;
    d.out_coloc_more_pip = pip.data(); d.out_coloc_more_set = set.data(); d.out_coloc_more_set_pip = set_pip.data();
    d.out_coloc_more_alpha = alpha.data(); d.out_coloc_more_V = V.data(); d.out_coloc_more_lse = lse.data();
    d.out_coloc_more_mass = mass.data(); d.out_coloc_more_purity = purity.data(); d.out_coloc_more_size = size.data();
    d.out_coloc_more_kept = kept.data(); d.out_coloc_more_sweeps = sweeps.data();
    d.coloc_p1 = p1 > 0 ? p1 : 1e-4;                                   // (a NaN compares false: coloc's defaults)
    d.coloc_p2 = p2 > 0 ? p2 : 1e-4;
    d.coloc_p12 = p12 > 0 ? p12 : 1e-5;
    d.out_coloc_pp = pp.data(); d.out_coloc_hit = hit.data(); d.out_coloc_hit_pp = hit_pp.data(); d.out_coloc_n = n.data();
    return 0;
}

int ColocRider::table(const WindowView& v, gauss_table** out)
{
    if (v.plain(out)) return -1;
    const SusieRider& s = susie;
    const SusieFit first = {s.pip.data(), s.set_pip.data(), s.alpha.data(), s.V.data(), s.lse.data(), s.mass.data(), s.purity.data(),
                            s.sweeps.data(), s.set.data(), s.size.data(), s.kept.data()};
    const ColocMore more = {traits.n_more, {pip.data(), set_pip.data(), alpha.data(), V.data(), lse.data(), mass.data(), purity.data(),
                                            sweeps.data(), set.data(), size.data(), kept.data()},
                            pp.data(), hit.data(), hit_pp.data(), n.data()};
    if (coloc_output(**out, v.measured, v.row_m, v.row_u, s.n_eff, s.tol_used, first, traits.n_more, traits.z.data(), traits.out_z.data(), more)) {
        gauss_table_free(*out); *out = nullptr;
        return -1;
    }
    return 0;
}
