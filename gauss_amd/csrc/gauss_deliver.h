// What rides on an imputation window's solve, and how its sections of the result block reach the caller.  Every section is described
// ONCE, in result_fields(): a field's place (from the layout structs of gauss_internal.h), its destination and the value it takes when
// the section is not fitted.  No HIP here: a host program compiles this header alone with GAUSS_LAYOUTS_ONLY (tests/test_deliver_host.py).
#pragma once
#include "gauss_internal.h"
#include "../../include/gauss_hip.h"
#include <cmath>
#include <cstring>
#include <vector>

using namespace gauss;

// Where a window's riders put their results (out_loo_* / out_slct_* / out_z_more of gauss_window_desc); every pointer is optional
struct RiderOuts {
    double *loo_z = nullptr, *loo_info = nullptr, *loo_t = nullptr;
    int32_t *slct_n = nullptr, *slct_idx = nullptr;
    double *slct_zin = nullptr, *slct_joint = nullptr, *slct_zc = nullptr, *slct_var = nullptr;
    double *cond_z = nullptr, *cond_var = nullptr;      // the imputed SNPs conditioned on the selection (gauss_window_desc.out_cond_*)
    double *cs_pip = nullptr, *cs_set_pip = nullptr, *cs_mass = nullptr, *cs_lse = nullptr;      // credible sets (gauss_window_desc.out_cs_*)
    int32_t *cs_set = nullptr, *cs_size = nullptr;
    double *susie_pip = nullptr, *susie_set_pip = nullptr, *susie_V = nullptr, *susie_lse = nullptr, *susie_mass = nullptr;      // the multi-causal fit
    double *susie_purity = nullptr, *susie_alpha = nullptr, *susie_mu = nullptr, *susie_sweeps = nullptr;                        // (gauss_window_desc.out_susie_*)
    int32_t *susie_set = nullptr, *susie_size = nullptr, *susie_kept = nullptr;
    double* susie_lbf = nullptr;
    // the further traits of the same fit (gauss_window_desc.out_coloc_more_*, a leading [k]) and the pairs (out_coloc_*)
    double *more_pip = nullptr, *more_set_pip = nullptr, *more_V = nullptr, *more_lse = nullptr, *more_mass = nullptr, *more_purity = nullptr;
    double *more_alpha = nullptr, *more_mu = nullptr, *more_lbf = nullptr, *more_sweeps = nullptr;
    int32_t *more_set = nullptr, *more_size = nullptr, *more_kept = nullptr, *more_status = nullptr;
    double *coloc_pp = nullptr, *coloc_hit_pp = nullptr;
    int32_t *coloc_hit = nullptr, *coloc_n = nullptr;
    double *xs_V = nullptr, *xs_purity = nullptr, *xs_mu = nullptr;      // the joint fit across studies, on a group's leader (gauss_window_desc.out_xs_*)
    int32_t* xs_n = nullptr;
    double *prs_beta = nullptr, *prs_delta = nullptr, *prs_br = nullptr, *prs_bg = nullptr, *prs_kkt = nullptr;      // polygenic score weights
    int32_t *prs_nnz = nullptr, *prs_sweeps = nullptr;                                                               // (gauss_window_desc.out_prs_*)
    double *lds_raw = nullptr, *lds_l2 = nullptr, *lds_mass = nullptr;      // LD scores of an LD window (gauss_window_desc.out_lds_*)
    double* z_more = nullptr;
    double *info_more = nullptr, *z_miss = nullptr, *info_miss = nullptr;      // (with a mask: gauss_window_desc.miss_more)
};

// What rides on an imputation window's solve (the sections of the result block: res_layout, gauss_internal.h).  A derived
// descriptor clears it with one assignment.
struct Riders {
    bool loo = false;                    // leave-one-out values of the measured SNPs (k_loo.hip)
    int slct_K = 0;                      // signal selection (k_slct.hip); 0: not asked
    std::vector<int> slct_forced;
    bool cond = false;                   // the imputed SNPs conditioned on the selection (k_cond.hip); needs slct_K
    bool cs = false;                     // credible sets of the selected signals (k_cs.hip); needs slct_K
    int susie_L = 0;                     // multi-causal fine-mapping (k_susie.hip): effects; 0: not asked
    bool susie_am = false;               // ... and its result section holds alpha and mu (out_susie_alpha / out_susie_mu ask)
    int susie_k = 0;                     // ... further traits fitted beside z1 (gauss_window_desc.coloc_traits_more)
    bool susie_lbf = false, coloc = false;      // ... the lbf rows are asked; the colocalisation of the traits' pairs is (k_coloc.hip)
    int xs_group = 0;                    // joint fit across studies (k_xsusie.hip): the group's id; 0: the window is in no group
    int xs_K = 0, xs_pos = 0, xs_lead = 0;      // ... the group's windows, this one's place among them (0: the leader), the leader's index in the job
    bool xs_mu = false;                  // ... the leader's section holds every study's mu (out_xs_mu asks)
    std::vector<int> xs_from_lead, xs_to_lead;  // ... Prob::xs_from_lead / xs_to_lead; empty: the same index
    int prs_n_s = 0, prs_n_lam = 0;      // polygenic score weights (k_prs.hip): the grid; 0: not asked
    bool lds = false;                    // LD scores of an LD window's measured SNPs (k_ldscore.hip)
    int lds_C = 0;                       // ... their annotation categories beside the plain score
    std::vector<int> lds_bp;             // ... Prob::lds_bp
    std::vector<double> lds_annot;       // ... Prob::lds_annot; empty: C = 0
    int traits_T = 0;                    // further traits (k_traits.hip); 0: not asked
    std::vector<double> traits_z;        // [Mld][T16]: the further traits' Z-scores, SNP-major, zero padded (the kernels' B operand)
    bool miss = false;                   // the traits came with a mask of missing SNPs (k_traits_miss.hip)
    int miss_n = 0;                      // set mask bits
    std::vector<int> miss_tab;           // Prob::miss_tab (MissTab, gauss_internal.h); empty: no mask
    RiderOuts out;
    bool needs_fused() const { return loo || traits_T > 0 || susie_L > 0; }      // it reads the rows of L^-1 that only the fused solve forms
    // (a peer of a group keeps its fit's state in the workspace and returns none of it: the joint fit's sections are the leader's)
    bool xs_peer() const { return xs_group != 0 && xs_pos > 0; }
    ResLayout layout(int n_rhs, int M, int U) const { return res_layout(n_rhs, M, U, loo, traits_T, slct_K, miss, miss_n, cond, cs, xs_peer() ? 0 : susie_L, susie_am, susie_lbf, susie_k, coloc, xs_group && xs_pos == 0 ? xs_K : 0, xs_mu, prs_n_s, prs_n_lam, lds, lds_C); }
};

// One field of a section: n values from res[off] on, `stride` doubles apart (1 but for the words of the prs cells).
//   d / i    where they go: as they are, or converted from the exact doubles that integers travel as.  Null: the caller did not ask;
//   unfit    the value in a window that is not finite, or -- the fit's sections -- not fitted;
//   raise    a status bit that a non-zero value raises (such a word has no destination), in *raise_at or, null, in the window's status.
struct Field { size_t off, n; double* d; int32_t* i; double unfit; size_t stride; int raise; int32_t* raise_at; };
struct Fields {
    std::vector<Field> f;
    void dbl(size_t off, size_t n, double* to, double unfit = NAN, size_t stride = 1) { if (n) f.push_back({off, n, to, nullptr, unfit, stride, 0, nullptr}); }
    void i32(size_t off, size_t n, int32_t* to, double unfit, size_t stride = 1) { if (n) f.push_back({off, n, nullptr, to, unfit, stride, 0, nullptr}); }
    void flag(size_t off, size_t n, int bit, int32_t* at = nullptr, size_t stride = 1) { if (n) f.push_back({off, n, nullptr, nullptr, 0.0, stride, bit, at}); }
};

// One fitted trait: its susie_layout at `at` and its lbf rows at `lbf`.  Trait 1's are the window's susie section and the head of
// susie_more; further trait t's (`more`) are block t of susie_more, and its outputs carry a leading [k]: every destination moves on by
// t times the field's length.
struct FitOuts { double *V, *lse, *mass, *purity, *pip, *set_pip, *alpha, *mu, *lbf, *sweeps; int32_t *size, *kept, *set, *status; };
inline void fit_fields(Fields& F, size_t at, size_t lbf, const Riders& rd, size_t T, const FitOuts& o, bool more, size_t t)
{
    const size_t L = (size_t)rd.susie_L, lt = L * T;
    const SusieLayout ql = susie_layout((int)T, rd.susie_L, rd.susie_am);
    auto to = [t](auto* p, size_t n) { return p ? p + t * n : p; };
    F.dbl(at + ql.V, L, to(o.V, L)); F.dbl(at + ql.lse, L, to(o.lse, L)); F.i32(at + ql.size, L, to(o.size, L), 0.0);
    F.dbl(at + ql.mass, L, to(o.mass, L)); F.dbl(at + ql.purity, L, to(o.purity, L)); F.i32(at + ql.kept, L, to(o.kept, L), 0.0);
    // fit [4]: sweeps run, the last delta, 1 when the sweeps ran out (the window's bit; a further trait's own word, out_coloc_more_status), unused
    F.dbl(at + ql.fit, 1, to(o.sweeps, 2), 0.0); F.dbl(at + ql.fit + 1, 1, o.sweeps ? to(o.sweeps, 2) + 1 : nullptr);
    F.flag(at + ql.fit + 2, 1, !more || o.status ? GAUSS_ST_SUSIE_NOCONV : 0, more ? to(o.status, 1) : nullptr); F.dbl(at + ql.fit + 3, 1, nullptr);
    F.dbl(at + ql.pip, T, to(o.pip, T)); F.i32(at + ql.set, T, to(o.set, T), -1.0); F.dbl(at + ql.set_pip, T, to(o.set_pip, T));
    if (rd.susie_am) { F.dbl(at + ql.alpha, lt, to(o.alpha, lt)); F.dbl(at + ql.mu, lt, to(o.mu, lt)); }
    if (rd.susie_lbf) F.dbl(lbf, lt, to(o.lbf, lt));
}

// One window's block (n_rhs = U: an imputation window's, or an LD window's with its LD scores), field by field, section by section (res_layout and the sub-layouts of gauss_internal.h):
// every double of the block belongs to exactly one field.
inline std::vector<Field> result_fields(int M, int U, const Riders& rd, const ResLayout& lay, double* out_z, double* out_info)
{
    Fields F;
    const RiderOuts& o = rd.out;
    const size_t m = (size_t)M, u = (size_t)U, T = m + u, K = (size_t)rd.slct_K;
    F.dbl(lay.z, u, out_z); F.dbl(lay.info, u, out_info);
    if (rd.loo) {                          // leave-one-out values of the measured SNPs (k_loo.hip)
        F.dbl(lay.loo, m, o.loo_z); F.dbl(lay.loo + m, m, o.loo_info); F.dbl(lay.loo + 2 * m, m, o.loo_t);
    }
    if (rd.traits_T) F.dbl(lay.traits, (size_t)rd.traits_T * u, o.z_more);      // the further traits (k_traits.hip)
    if (rd.miss) {                         // ... that lack some measured SNPs (k_traits_miss.hip)
        F.dbl(lay.traits_info, (size_t)rd.traits_T * u, o.info_more);
        F.dbl(lay.traits_miss, (size_t)rd.miss_n, o.z_miss); F.dbl(lay.traits_miss + rd.miss_n, (size_t)rd.miss_n, o.info_miss);
    }
    if (K) {                               // signal selection (k_slct.hip).  Nothing selected: n = 0, no skipped SNP, indices -1
        const SlctLayout sl = slct_layout(M, rd.slct_K);
        const size_t at = lay.slct;
        F.i32(at + sl.n, 1, o.slct_n, 0.0); F.flag(at + sl.skipped, 1, GAUSS_ST_SLCT_SKIPPED); F.i32(at + sl.idx, K, o.slct_idx, -1.0);
        F.dbl(at + sl.zin, K, o.slct_zin); F.dbl(at + sl.joint, K, o.slct_joint); F.dbl(at + sl.zc, m, o.slct_zc); F.dbl(at + sl.var, m, o.slct_var);
    }
    if (rd.cond) { F.dbl(lay.cond, u, o.cond_z); F.dbl(lay.cond + u, u, o.cond_var); }      // conditioned on the selection (k_cond.hip)
    if (rd.cs) {                           // credible sets of the selected signals (k_cs.hip).  No sets: size 0, set -1
        const CsLayout cl = cs_layout((int)T, rd.slct_K);
        const size_t at = lay.cs;
        F.i32(at + cl.size, K, o.cs_size, 0.0); F.dbl(at + cl.mass, K, o.cs_mass); F.dbl(at + cl.lse, K, o.cs_lse);
        F.dbl(at + cl.pip, T, o.cs_pip); F.i32(at + cl.set, T, o.cs_set, -1.0); F.dbl(at + cl.set_pip, T, o.cs_set_pip);
    }
    if (rd.susie_L && !rd.xs_peer()) {     // the multi-causal fit (k_susie.hip); for a group's leader the joint fit (k_xsusie.hip)
        // not fitted: NaN, size 0, kept 0, set -1, no sweep; every pair NaN, hit -1, n 0; no joint candidate
        const size_t L = (size_t)rd.susie_L, lt = L * T, at = lay.susie_more;
        const SusieMoreLayout ml = susie_more_layout((int)T, rd.susie_L, rd.susie_am, rd.susie_lbf, rd.susie_k, rd.coloc);
        fit_fields(F, lay.susie, at + ml.lbf, rd, T, {o.susie_V, o.susie_lse, o.susie_mass, o.susie_purity, o.susie_pip, o.susie_set_pip, o.susie_alpha,
                                                      o.susie_mu, o.susie_lbf, o.susie_sweeps, o.susie_size, o.susie_kept, o.susie_set, nullptr}, false, 0);
        for (size_t t = 0; t < (size_t)rd.susie_k; t++)
            fit_fields(F, at + ml.trait + t * ml.one, at + ml.trait + t * ml.one + ml.tlbf, rd, T,
                       {o.more_V, o.more_lse, o.more_mass, o.more_purity, o.more_pip, o.more_set_pip, o.more_alpha, o.more_mu, o.more_lbf, o.more_sweeps,
                        o.more_size, o.more_kept, o.more_set, o.more_status}, true, t);
        if (rd.coloc) {                    // the pairs of fitted traits (k_coloc.hip)
            const size_t np = (size_t)(rd.susie_k + 1) * rd.susie_k / 2, ll = L * L;
            F.dbl(at + ml.pp, 5 * np * ll, o.coloc_pp); F.i32(at + ml.hit, np * ll, o.coloc_hit, -1.0);
            F.dbl(at + ml.hit_pp, np * ll, o.coloc_hit_pp); F.i32(at + ml.n, np, o.coloc_n, 0.0);
        }
        if (lay.prs > lay.xs) {            // a group's leader: what the joint fit holds per study (k_xsusie.hip)
            const XsLayout xl = xs_layout(rd.xs_K, rd.susie_L, (int)T, rd.xs_mu);
            const size_t kl = (size_t)rd.xs_K * L;
            F.dbl(lay.xs + xl.V, kl, o.xs_V); F.dbl(lay.xs + xl.purity, kl, o.xs_purity); F.i32(lay.xs + xl.n, 1, o.xs_n, 0.0);
            if (rd.xs_mu) F.dbl(lay.xs + xl.mu, kl * T, o.xs_mu);
        }
    }
    if (rd.prs_n_s) {                      // polygenic score weights (k_prs.hip).  No fit: nnz 0, no sweep, no flag
        const size_t nc = (size_t)rd.prs_n_s * rd.prs_n_lam;
        const PrsLayout ql = prs_layout(M, rd.prs_n_s, rd.prs_n_lam);
        const size_t at = lay.prs + ql.cell;
        F.i32(at + PRS_NNZ, nc, o.prs_nnz, 0.0, PRS_CELL); F.i32(at + PRS_SWEEPS, nc, o.prs_sweeps, 0.0, PRS_CELL);
        F.dbl(at + PRS_DELTA, nc, o.prs_delta, NAN, PRS_CELL); F.dbl(at + PRS_BR, nc, o.prs_br, NAN, PRS_CELL);
        F.dbl(at + PRS_BG, nc, o.prs_bg, NAN, PRS_CELL); F.dbl(at + PRS_KKT, nc, o.prs_kkt, NAN, PRS_CELL);
        F.flag(at + PRS_NOCONV, nc, GAUSS_ST_PRS_NOCONV, nullptr, PRS_CELL); F.dbl(at + PRS_NOCONV + 1, nc, nullptr, NAN, PRS_CELL);
        F.dbl(lay.prs + ql.beta, nc * m, o.prs_beta);
    }
    if (rd.lds) {                          // LD scores of an LD window's measured SNPs (k_ldscore.hip)
        const LdsLayout ll = lds_layout(M, rd.lds_C);
        const size_t n = (size_t)(1 + rd.lds_C) * m;
        F.dbl(lay.lds + ll.raw, n, o.lds_raw); F.dbl(lay.lds + ll.l2, n, o.lds_l2); F.dbl(lay.lds + ll.mass, n, o.lds_mass);
    }
    return F.f;
}

// The fields that start in res[from, to) take their not-fitted values
inline void fill_unfit(double* res, const std::vector<Field>& fields, size_t from, size_t to)
{
    for (const Field& x : fields)
        if (x.off >= from && x.off < to)
            for (size_t e = 0; e < x.n; e++) res[x.off + e * x.stride] = x.unfit;
}
// Every field to where the caller asked for it; returns the status bits its flag words raise for the window
inline int copy_out(const double* res, const std::vector<Field>& fields)
{
    int bits = 0;
    for (const Field& x : fields) {
        const double* const s = res + x.off;
        if (x.d && x.stride == 1) memcpy(x.d, s, sizeof(double) * x.n);
        else if (x.d) for (size_t e = 0; e < x.n; e++) x.d[e] = s[e * x.stride];
        else if (x.i) for (size_t e = 0; e < x.n; e++) x.i[e] = (int32_t)s[e * x.stride];
        else for (size_t e = 0; e < x.n; e++) if (x.raise && s[e * x.stride] != 0.0) *(x.raise_at ? x.raise_at : &bits) |= x.raise;
    }
    return bits;
}

// One imputation window's block `res` to the caller's memory; returns the window's status bits.  bits: 0, or what the repair left
// (GAUSS_ST_CLAMPED or GAUSS_ST_NONFINITE); repaired: this window, or a member of its group of the joint fit, went through the repair.
// Not finite: the reference's eigen-solver / LU propagate non-finite values to every output.  A repaired B11 (MakePosDef) is no ground
// for the multi-causal fit, and the clamp path's stand-alone solve forms no rows of the inverse: the fit's sections are filled as not
// fitted and every member of the group says GAUSS_ST_SUSIE_NOFIT.
inline int deliver_window(double* res, int M, int U, const Riders& rd, double* out_z, double* out_info, int bits, bool repaired)
{
    const ResLayout lay = rd.layout(U, M, U);
    const std::vector<Field> fields = result_fields(M, U, rd, lay, out_z, out_info);
    if (bits & GAUSS_ST_NONFINITE) fill_unfit(res, fields, 0, lay.count);
    else if ((rd.susie_L || rd.xs_peer()) && repaired) { fill_unfit(res, fields, lay.susie, lay.prs); bits |= GAUSS_ST_SUSIE_NOFIT; }
    if (rd.out.more_status && rd.susie_L && !rd.xs_peer())
        for (int t = 0; t < rd.susie_k; t++) rd.out.more_status[t] = bits & (GAUSS_ST_SUSIE_NOFIT | GAUSS_ST_NONFINITE);
    return bits | copy_out(res, fields);
}
