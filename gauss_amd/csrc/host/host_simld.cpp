// libgauss_host.so -- simulateLD() (simulateLD.cpp:34-252): the LD of a simulated mixed-ancestry cohort.  The draws are made on
// the host with a seeded std::mt19937 (the reference seeds it from std::random_device: no two calls agree); the resampled
// genotype matrix is never formed -- gauss_ld_resampled_rows packs the drawn columns of each row on the GPU (k_simld.hip).
#include "host_internal.h"

#include <random>

namespace {

// uniform_int_distribution<>(0, n - 1) on a 32-bit generator as libstdc++ >= 11 draws it: Lemire's nearly-divisionless method on
// a 64-bit product, rejecting while the low word is below (2^32 - n) mod n.  Written out, it gives the same draws everywhere.
inline uint32_t bounded_draw(std::mt19937& gen, uint32_t n)
{
    uint64_t prod = (uint64_t)(uint32_t)gen() * n;
    uint32_t low = (uint32_t)prod;
    if (low < n) {
        const uint32_t threshold = (uint32_t)(0u - n) % n;
        while (low < threshold) {
            prod = (uint64_t)(uint32_t)gen() * n;
            low = (uint32_t)prod;
        }
    }
    return (uint32_t)(prod >> 32);
}

struct SimDraws {
    std::vector<int> pops;              // the flagged populations (panel indices, panel order)
    std::vector<int32_t> counts;        // draws of each
    std::vector<int32_t> pop, sample;   // draw k: sample `sample[k]` of flagged population `pop[k]` (index into pops)
    uint32_t seed = 0;
};

// simulateLD.cpp:134-151: every population of the weight map, in PANEL order, gets (int)(w * sim_size) draws (fp64 on the raw
// weight, no normalising), each uniform_int_distribution<>(0, n_k - 1) on one generator shared by all populations.  What the
// reference leaves undefined is refused.
int simulate_draws(const Args& a, int64_t sim_size, int64_t seed, SimDraws& d)
{
    if (sim_size < 1 || sim_size > INT32_MAX) return herr("simulateLD: sim_size must be in 1 .. %d (got %lld)", INT32_MAX, (long long)sim_size);
    if (seed < -1 || seed > (int64_t)UINT32_MAX) return herr("simulateLD: seed must be -1 or in [0, 2^32) (got %lld)", (long long)seed);
    int64_t total = 0;
    for (int k = 0; k < a.num_pops; k++) {
        if (!a.pop_flag_vec[(size_t)k]) continue;
        const std::string& pop = a.ref_pop_vec[(size_t)k];
        const double w = a.pop_wgt_map.at(pop);
        // a negative count would move the reference's column counter backwards (simulateLD.cpp:176)
        if (!std::isfinite(w) || w < 0) return herr("simulateLD: the weight of population %s is %g; weights must be finite and >= 0", pop.c_str(), w);
        const double x = w * (double)sim_size;                            // simulateLD.cpp:141
        if (x >= 2147483648.0)
            return herr("simulateLD: population %s asks for %.17g draws, more than sim_size = %lld", pop.c_str(), x, (long long)sim_size);
        const int c = (int)x;
        if (c > 0 && a.ref_pop_size_vec[(size_t)k] < 1) return herr("simulateLD: population %s has no samples to draw from", pop.c_str());
        d.pops.push_back(k);
        d.counts.push_back(c);
        total += c;
    }
    // geno_mat has sim_size columns: more draws would be written past its end (simulateLD.cpp:161-179)
    if (total > sim_size)
        return herr("simulateLD: the weights ask for %lld draws in all (sum of (int)(weight * sim_size)), more than sim_size = %lld",
                    (long long)total, (long long)sim_size);
    d.seed = seed < 0 ? (uint32_t)std::random_device()() : (uint32_t)seed;
    std::mt19937 gen(d.seed);
    d.pop.reserve((size_t)total);
    d.sample.reserve((size_t)total);
    for (size_t q = 0; q < d.pops.size(); q++) {
        const uint32_t n = (uint32_t)a.ref_pop_size_vec[(size_t)d.pops[q]];
        for (int j = 0; j < d.counts[q]; j++) {
            d.pop.push_back((int32_t)q);
            d.sample.push_back((int32_t)bounded_draw(gen, n));
        }
    }
    return 0;
}

// named members shared by both entry points: counts [P x 1], draws [n_drawn x 2] (flagged population, sample), seed [1 x 1]
void put_draws(gauss_table& t, const SimDraws& d)
{
    t.put_named("counts", (int)d.counts.size(), 1, std::vector<double>(d.counts.begin(), d.counts.end()));
    const size_t n = d.pop.size();
    std::vector<double> dr(2 * n);
    for (size_t k = 0; k < n; k++) { dr[k] = d.pop[k]; dr[n + k] = d.sample[k]; }
    t.put_named("draws", (int)n, 2, std::move(dr));
    t.put_named("seed", 1, 1, std::vector<double>(1, (double)d.seed));
}

}  // namespace

extern "C" {

int gauss_host_simulate_draws(const char* reference_pop_desc_file, const char* const* pop_names, const double* pop_wgts, int n_pop_wgt,
                              int64_t sim_size, int64_t seed, gauss_table** out)
{
    if (!out || !reference_pop_desc_file || n_pop_wgt < 0 || (n_pop_wgt > 0 && (!pop_names || !pop_wgts))) return herr("bad arguments");
    *out = nullptr;
    Args a;
    a.reference_pop_desc_file = reference_pop_desc_file;
    if (read_ref_desc(a)) return -1;
    set_pop_wgt_map(a, pop_names, pop_wgts, n_pop_wgt);
    init_pop_flag_wgt_vec(a);
    SimDraws d;
    if (simulate_draws(a, sim_size, seed, d)) return -1;
    std::unique_ptr<gauss_table> t(new gauss_table());
    t->add("pop", GAUSS_COL_STR); t->add("n", GAUSS_COL_INT); t->add("count", GAUSS_COL_INT);
    for (size_t q = 0; q < d.pops.size(); q++) {
        t->cols[0].s.push_back(a.ref_pop_vec[(size_t)d.pops[q]]);
        t->cols[1].i.push_back(a.ref_pop_size_vec[(size_t)d.pops[q]]);
        t->cols[2].i.push_back(d.counts[q]);
    }
    put_draws(*t, d);
    *out = t.release();
    return 0;
}

int gauss_host_simulateLD(gauss_ctx* ctx, int chr, int64_t start_bp, int64_t end_bp, const char* const* pop_names, const double* pop_wgts,
                          int n_pop_wgt, int64_t sim_size, const char* input_file, const char* reference_index_file,
                          const char* reference_data_file, const char* reference_pop_desc_file, double af1_cutoff, int64_t seed,
                          gauss_table** out)
{
    if (!ctx || !out) return herr("bad arguments");
    *out = nullptr;
    LdRows s;
    if (computeld_rows(ctx, chr, start_bp, end_bp, pop_names, pop_wgts, n_pop_wgt, input_file, reference_index_file, reference_data_file,
                       reference_pop_desc_file, af1_cutoff, s)) return -1;
    SimDraws d;
    if (simulate_draws(s.a, sim_size, seed, d)) return -1;
    // the draws index the selected populations, the same list and order the rows' pop_off describes
    const int P = s.n_pop();
    if ((int)d.pops.size() != P) return herr("simulateLD: %d weighted populations but %d selected for the rows", (int)d.pops.size(), P);
    for (int q = 0; q < P; q++)
        if (s.pop_off[(size_t)q + 1] - s.pop_off[(size_t)q] != s.a.ref_pop_size_vec[(size_t)d.pops[(size_t)q]])
            return herr("simulateLD: population %s has %d samples in the rows, %d in the description file", s.a.ref_pop_vec[(size_t)d.pops[(size_t)q]].c_str(),
                        s.pop_off[(size_t)q + 1] - s.pop_off[(size_t)q], s.a.ref_pop_size_vec[(size_t)d.pops[(size_t)q]]);
    const int M = s.M;
    std::unique_ptr<gauss_table> t = std::move(s.t);
    t->matrix.assign((size_t)M * M, 0.0);
    t->matrix_n = M;
    if (gauss_ld_resampled_rows(ctx, s.store, s.ld, s.geno_fmt, s.row_ptr(), M, s.pop_off.data(), s.src_off_ptr(), P, d.pop.data(), d.sample.data(),
                                (int64_t)d.pop.size(), sim_size, 1.0, s.on_device, t->matrix.data()) != 0)
        return herr("%s", gauss_last_error());
    put_draws(*t, d);
    *out = t.release();
    return 0;
}

}  // extern "C"
