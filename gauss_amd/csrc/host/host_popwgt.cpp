// libgauss_host.so -- afmix() / cpw2() (afmix.cpp:30-215, cpw2.cpp:31-211): the study's allele frequencies against the panel's
// per-population ones.  The host reads the study (ReadInputAf), merges the panel index (ReadReferenceIndexAll), lists the measured
// SNPs in map order and lays their AF rows out interval-major; gauss_pop_weights (libgauss_hip) computes every interval's W_i; the
// host sums them in interval order and rounds (afmix.cpp:192-211).
#include "host_internal.h"

namespace {

struct PwInputs {
    Args a;
    SnpMap m;
    std::vector<Snp*> measured;        // type-1 SNPs, map order (afmix.cpp:68-73)
    int interval = 1000;
    int P = 0;
    std::vector<int64_t> off;          // [interval + 1] rows of each interval
    std::vector<double> x;             // [S x (P + 1)] interval-major rows [af1study, AF_0 .. AF_(P-1)], cpw2-transformed
};

inline double pw_value(int kind, double v) { return kind == GAUSS_KIND_CPW2 ? std::asin(std::sqrt(v)) : v; }   // cpw2.cpp:147, 166

int popwgt_inputs(int kind, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                  const char* reference_pop_desc_file, int interval, PwInputs& in)
{
    if (kind != GAUSS_KIND_AFMIX && kind != GAUSS_KIND_CPW2) return herr("kind %d is neither GAUSS_KIND_AFMIX nor GAUSS_KIND_CPW2", kind);
    if (files_ok({input_file, reference_data_file, reference_pop_desc_file})) return -1;
    Args& a = in.a;
    a.input_file = input_file; a.reference_index_file = reference_index_file ? reference_index_file : "";
    a.reference_data_file = reference_data_file; a.reference_pop_desc_file = reference_pop_desc_file;
    in.interval = interval > 0 ? interval : 1000;                              // afmix.cpp:47-51 (R NULL -> 1000)
    if (!reference_index_file && !PackedPanel::is_packed(reference_data_file))
        return herr("reference_index_file is NULL and '%s' is not a packed panel", reference_data_file);
    if (open_panel_all_pops(a, reference_index_file)) return -1;              // every population of the description file
    in.P = a.num_pops;
    if (ReadInputAf(in.m, a)) return -1;
    if (ReadReferenceIndex(in.m, a, true)) return -1;
    for (auto& kv : in.m) if (kv.second->type == 1) in.measured.push_back(kv.second.get());
    const int64_t S = (int64_t)in.measured.size();
    const int iv = in.interval;
    if (S < iv)
        return herr("ERROR: %lld measured SNPs and interval = %d: interval %lld would hold no SNP (afmix / cpw2 need at least `interval` "
                    "measured SNPs)", (long long)S, iv, (long long)S);
    // interval i holds the measured SNPs i, i + interval, i + 2 interval, ... (afmix.cpp:136-145)
    in.off.assign((size_t)iv + 1, 0);
    for (int i = 0; i < iv; i++) in.off[(size_t)i + 1] = in.off[(size_t)i] + (S - i + iv - 1) / iv;
    const int nc = in.P + 1;
    in.x.assign((size_t)S * nc, 0.0);
    auto row_of = [&](int64_t j) { return in.off[(size_t)(j % iv)] + j / iv; };
    if (a.pk) {
        for (int64_t j = 0; j < S; j++) {
            double* r = in.x.data() + (size_t)row_of(j) * nc;
            const double* af = a.pk->af(in.measured[(size_t)j]->fpos);
            r[0] = pw_value(kind, in.measured[(size_t)j]->af1study);
            for (int p = 0; p < in.P; p++) r[1 + p] = pw_value(kind, af[p]);
        }
        return 0;
    }
    // text panel: the P allele frequencies after the P genotype strings of every SNP's data line (afmix.cpp:148-168); the lines
    // are independent, so blocks of SNPs (panel order) are read by several threads, each with its own reader
    const int64_t BLK = 256;
    const int nblk = (int)((S + BLK - 1) / BLK);
    std::atomic<int> failed{0};
    std::vector<BgzfReader> readers((size_t)std::max(1, host_threads()));
    for (BgzfReader& fp : readers) if (!fp.open(a.reference_data_file)) return herr("ERROR: can't open reference data file '%s'", a.reference_data_file.c_str());
    std::atomic<int> next{0};
    auto work = [&](BgzfReader& fp) {
        std::string line;
        for (int b = next.fetch_add(1); b < nblk; b = next.fetch_add(1))
            for (int64_t j = (int64_t)b * BLK; j < std::min(S, (int64_t)(b + 1) * BLK); j++) {
                Snp& s = *in.measured[(size_t)j];
                line.clear();
                fp.seek(s.fpos);
                if (fp.getline(line) == -2) { failed = 1; return; }
                Tok t(line);
                for (int k = 0; k < in.P; k++) { const char* q; int n; t.next(q, n); }       // the genotype strings
                double* r = in.x.data() + (size_t)row_of(j) * nc;
                r[0] = pw_value(kind, s.af1study);
                for (int p = 0; p < in.P; p++) {
                    double af = 0.0;            // a failed extraction leaves 0 (C++11 num_get), as in load_line
                    t.dbl(af);
                    r[1 + p] = pw_value(kind, af);
                }
            }
    };
    std::vector<std::thread> th;
    for (size_t k = 1; k < readers.size(); k++) th.emplace_back(work, std::ref(readers[k]));
    work(readers[0]);
    for (std::thread& t : th) t.join();
    if (failed) return herr("Error: can't read reference data file '%s'", a.reference_data_file.c_str());
    return 0;
}

int run_popwgt(gauss_ctx* ctx, int kind, const char* input_file, const char* reference_index_file, const char* reference_data_file,
               const char* reference_pop_desc_file, int interval, gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    *out = nullptr;
    PwInputs in;
    if (popwgt_inputs(kind, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, interval, in)) return -1;
    const int iv = in.interval, P = in.P;
    const int64_t S = (int64_t)in.measured.size();
    std::vector<double> w_int((size_t)iv * P);
    std::vector<int32_t> status((size_t)iv);
    if (gauss_pop_weights(ctx, in.x.data(), in.off.data(), iv, P, in.a.min_abs_eig, w_int.data(), status.data()) != GAUSS_OK)
        return herr("%s", gauss_last_error());
    // W = sum_i W_i / interval, in interval order (afmix.cpp:192-195); then w < 0 -> 0, else rounded to 3 decimals (:198-205)
    std::vector<double> W((size_t)P, 0.0);
    for (int i = 0; i < iv; i++)
        for (int p = 0; p < P; p++) W[(size_t)p] = W[(size_t)p] + w_int[(size_t)i * P + p] / iv;
    std::unique_ptr<gauss_table> t(new gauss_table());
    const bool afmix = kind == GAUSS_KIND_AFMIX;   // afmix: sup.pop pop wgt; cpw2: pop wgt
    if (afmix) t->add("sup.pop", GAUSS_COL_STR);
    t->add("pop", GAUSS_COL_STR);
    t->add("wgt", GAUSS_COL_DBL);
    const int c0 = afmix ? 1 : 0;
    for (int p = 0; p < P; p++) {
        const double w = W[(size_t)p] < 0 ? 0.0 : std::floor(W[(size_t)p] * 1000 + 0.5) / 1000;
        if (w > 0) {                               // afmix.cpp:91-99: only populations with a positive weight (NaN drops out)
            if (afmix) t->cols[0].s.push_back(in.a.ref_sup_pop_vec[(size_t)p]);
            t->cols[(size_t)c0].s.push_back(in.a.ref_pop_vec[(size_t)p]);
            t->cols[(size_t)c0 + 1].d.push_back(w);
        }
    }
    t->put_named("w_raw", P, 1, W);
    std::vector<double> wi((size_t)iv * P), st((size_t)iv);
    for (int i = 0; i < iv; i++) {
        for (int p = 0; p < P; p++) wi[(size_t)p * iv + i] = w_int[(size_t)i * P + p];       // column-major
        st[(size_t)i] = status[(size_t)i];
    }
    t->put_named("w_interval", iv, P, std::move(wi));
    t->put_named("status", iv, 1, std::move(st));
    int n_nan = 0;
    for (int i = 0; i < iv; i++) n_nan += (status[(size_t)i] & GAUSS_ST_NONFINITE) ? 1 : 0;
    if (n_nan) {
        char msg[512];
        if (S < 2 * (int64_t)iv)
            snprintf(msg, sizeof(msg), "%lld measured SNPs and interval = %d: %lld interval(s) hold a single SNP, whose covariance is 0/0 = NaN, "
                     "so every weight is NaN and no population is returned (as in the reference)", (long long)S, iv, (long long)(2 * (int64_t)iv - S));
        else
            snprintf(msg, sizeof(msg), "%d of %d intervals gave NaN weights (non-finite allele frequencies or a failed eigen-solve): "
                     "every weight is NaN and no population is returned", n_nan, iv);
        t->messages.push_back(msg);
    }
    *out = t.release();
    return 0;
}

}  // namespace

extern "C" {

int gauss_host_afmix(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                     const char* reference_pop_desc_file, int interval, gauss_table** out)
{
    return run_popwgt(ctx, GAUSS_KIND_AFMIX, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, interval, out);
}

int gauss_host_cpw2(gauss_ctx* ctx, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                    const char* reference_pop_desc_file, int interval, gauss_table** out)
{
    return run_popwgt(ctx, GAUSS_KIND_CPW2, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, interval, out);
}

int gauss_host_popwgt_inputs(int kind, const char* input_file, const char* reference_index_file, const char* reference_data_file,
                             const char* reference_pop_desc_file, int interval, gauss_table** out)
{
    if (!out) return herr("bad arguments");
    *out = nullptr;
    PwInputs in;
    if (popwgt_inputs(kind, input_file, reference_index_file, reference_data_file, reference_pop_desc_file, interval, in)) return -1;
    std::unique_ptr<gauss_table> t(new gauss_table());
    add_ident_columns(*t, in.measured);
    Column& af = t->add("af1study", GAUSS_COL_DBL);
    for (Snp* s : in.measured) af.d.push_back(s->af1study);
    const int64_t S = (int64_t)in.measured.size();
    const int nc = in.P + 1;
    std::vector<double> x((size_t)S * nc);
    for (int64_t r = 0; r < S; r++)
        for (int c = 0; c < nc; c++) x[(size_t)c * S + r] = in.x[(size_t)r * nc + c];         // column-major
    t->put_named("x", (int)S, nc, std::move(x));
    std::vector<double> off(in.off.begin(), in.off.end());
    t->put_named("interval_off", (int)in.off.size(), 1, std::move(off));
    *out = t.release();
    return 0;
}

}  // extern "C"
