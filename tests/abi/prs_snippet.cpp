// The Rcpp-side code of INTEGRATION.md section 5m7 (polygenic score weights of a window), compiled against include/gauss_hip.h by
// tests/test_prs_host.py: keeps the documented fields in step with the C ABI.
#include <cmath>
#include <cstdint>
#include <vector>

#include "gauss_hip.h"

int prs_window(gauss_ctx* ctx, gauss_window_desc w, int M, double n_study, std::vector<double>& beta, std::vector<int32_t>& nnz,
               std::vector<double>& r2, bool& converged)
{
  const std::vector<double> s = {0.2, 0.5, 0.9, 1.0};                 // 1 .. GAUSS_PRS_MAX_S shrinkage values in (0, 1]
  std::vector<double> lam;                                            // 1 .. GAUSS_PRS_MAX_LAM penalties, in the order a chain takes them
  for (int k = 0; k < 20; k++) lam.push_back(std::exp(std::log(0.1) + (std::log(0.001) - std::log(0.1)) * k / 19.0));
  const size_t nc = s.size() * lam.size();
  std::vector<double> br(nc), bg(nc);
  int32_t status = 0;
  beta.assign(nc * M, 0.0);  nnz.assign(nc, 0);  r2.assign(nc, 0.0);
  w.prs_n_s = (int)s.size();  w.prs_s = s.data();                     // prs_n_s > 0 switches the fit on
  w.prs_n_lam = (int)lam.size();  w.prs_lam = lam.data();
  w.prs_n = n_study;                                                  // r = z / sqrt(n - 2 + z^2)
  w.prs_tol = 1e-4;  w.prs_max_sweeps = 100;                          // 1 .. GAUSS_PRS_MAX_SWEEPS
  w.out_prs_beta = beta.data();  w.out_prs_nnz = nnz.data();  w.out_prs_br = br.data();  w.out_prs_bg = bg.data();      // every output is optional
  w.out_status = &status;
  const int rc = gauss_impute_window(ctx, &w);
  converged = !(status & GAUSS_ST_PRS_NOCONV);                        // else: some cell holds the values of its last sweep
  for (size_t c = 0; c < nc; c++) r2[c] = bg[c] > 0 ? br[c] * br[c] / bg[c] : 0.0;      // the in-sample predicted R^2 of cell c
  return rc;
  // cell c = i_s * n_lam + i_lam; beta[c * M + m] is the weight of measured SNP m (standardised-genotype units) at (s[i_s], lam[i_lam]).
}
