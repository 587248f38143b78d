// The Rcpp-side code of INTEGRATION.md section 5m3 (credible sets of the selected signals), compiled against include/gauss_hip.h by
// tests/test_cs_host.py: keeps the documented fields in step with the C ABI.
#include <cstdint>
#include <vector>

#include "gauss_hip.h"

int cs_window(gauss_ctx* ctx, gauss_window_desc w, int M, int U, double chi2_stop, std::vector<double>& pip, std::vector<int32_t>& set,
              std::vector<double>& set_pip, std::vector<int32_t>& size, std::vector<double>& mass, int32_t& n_sel)
{
  const int K = 32;
  const double collin = 0.9;
  std::vector<int32_t> idx(K, -1);
  std::vector<double> lse(K);
  pip.assign(M + U, 0.0);  set.assign(M + U, -1);  set_pip.assign(M + U, 0.0);  size.assign(K, 0);  mass.assign(K, 0.0);
  w.slct_max = K;  w.slct_chi2_stop = chi2_stop;
  w.slct_min_var_frac = 1.0 - collin / ((1.0 + w.lambda) * (1.0 + w.lambda));   // the measured candidates' guard
  w.out_slct_n = &n_sel;  w.out_slct_idx = idx.data();
  w.cond_min_var_frac = 1.0 - collin;                                           // the imputed candidates' guard (read without out_cond_*)
  w.cs_coverage = 0.95;  w.cs_prior_var = 25.0;                                 // rho in (0, 1], omega > 0: anything else is refused
  w.out_cs_pip = pip.data();  w.out_cs_set = set.data();  w.out_cs_set_pip = set_pip.data();      // any one switches the computation on
  w.out_cs_size = size.data();  w.out_cs_mass = mass.data();  w.out_cs_lse = lse.data();
  return gauss_impute_window(ctx, &w);
  // candidate c < M is measured SNP c, candidate M + u imputed SNP u.  set[c]: the 0-based signal whose credible set holds the SNP
  // (-1: none), set_pip[c] its probability there, pip[c] its inclusion probability over all signals; size[a] / mass[a]: signal a's set.
}
