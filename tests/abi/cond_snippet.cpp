// The Rcpp-side code of INTEGRATION.md section 5m2 (imputed SNPs conditioned on the selected signals), compiled against
// include/gauss_hip.h by tests/test_cond_host.py: keeps the documented fields in step with the C ABI.
#include <cstdint>
#include <vector>

#include "gauss_hip.h"

int cond_window(gauss_ctx* ctx, gauss_window_desc w, int M, int U, const std::vector<int32_t>& forced, double chi2_stop,
                std::vector<double>& cond_z, std::vector<double>& cond_var, std::vector<int32_t>& idx, int32_t& n_sel)
{
  const int K = 32;
  const double collin = 0.9;
  std::vector<double> zin(K), joint(K), zc(M), var_left(M);
  idx.assign(K, -1);  cond_z.assign(U, 0.0);  cond_var.assign(U, 0.0);
  w.slct_max = K;  w.slct_chi2_stop = chi2_stop;
  w.slct_min_var_frac = 1.0 - collin / ((1.0 + w.lambda) * (1.0 + w.lambda));   // measured SNPs: the ridge caps what a twin explains
  w.slct_forced = forced.empty() ? nullptr : forced.data();  w.n_slct_forced = (int)forced.size();
  w.out_slct_n = &n_sel;  w.out_slct_idx = idx.data();  w.out_slct_zin = zin.data();  w.out_slct_joint = joint.data();
  w.out_slct_zc = zc.data();  w.out_slct_var = var_left.data();
  w.cond_min_var_frac = 1.0 - collin;                                           // imputed SNPs: it does not; no (1 + lambda)^2 here
  w.out_cond_z = cond_z.data();  w.out_cond_var = cond_var.data();              // either one switches the computation on
  return gauss_impute_window(ctx, &w);
  // cond_z[u]: z of imputed SNP u given the selected SNPs, NaN where they leave it less than 1 - collin of its variance;
  // cond_var[u]: that share.  Nothing selected: cond_z has the bits of out_z, cond_var is 1.
}
