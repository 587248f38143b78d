// The Rcpp-side code of INTEGRATION.md section 5m4 (multi-causal fine-mapping of a window), compiled against include/gauss_hip.h by
// tests/test_susie_host.py: keeps the documented fields in step with the C ABI.
#include <cstdint>
#include <vector>

#include "gauss_hip.h"

int susie_window(gauss_ctx* ctx, gauss_window_desc w, int M, int U, std::vector<double>& pip, std::vector<int32_t>& set,
                 std::vector<double>& set_pip, std::vector<int32_t>& kept, std::vector<double>& purity, bool& converged, bool& fitted)
{
  const int L = 10;
  std::vector<double> sweeps(2);
  int32_t status = 0;
  pip.assign(M + U, 0.0);  set.assign(M + U, -1);  set_pip.assign(M + U, 0.0);  kept.assign(L, 0);  purity.assign(L, 0.0);
  w.susie_L = L;                                                      // 1 .. GAUSS_SUSIE_MAX_L switches the fit on
  w.susie_coverage = 0.95;  w.susie_prior_var = 25.0;                 // rho in (0, 1], omega > 0 in z units
  w.susie_tol = 1e-4;  w.susie_max_sweeps = 100;  w.susie_min_abs_corr = 0.5;
  w.susie_estimate_var = 1;  w.susie_measured_only = 0;               // 1: plain SuSiE-RSS on the measured SNPs
  w.out_susie_pip = pip.data();  w.out_susie_set = set.data();  w.out_susie_set_pip = set_pip.data();      // every output is optional
  w.out_susie_kept = kept.data();  w.out_susie_purity = purity.data();  w.out_susie_sweeps = sweeps.data();
  w.out_status = &status;
  const int rc = gauss_impute_window(ctx, &w);
  converged = !(status & GAUSS_ST_SUSIE_NOCONV);                      // else: the values of the last sweep
  fitted = !(status & (GAUSS_ST_SUSIE_NOFIT | GAUSS_ST_NONFINITE));   // a window MakePosDef repairs is not fitted: NaN, set -1
  return rc;
  // candidate c < M is measured SNP c, candidate M + u imputed SNP u.  set[c]: the 0-based effect whose kept set holds the SNP (-1: none),
  // set_pip[c] its probability there, pip[c] its inclusion probability over all effects; kept[l] / purity[l]: effect l's set.
}
