// The Rcpp-side code of INTEGRATION.md section 5m6 (joint fine-mapping across studies), compiled against include/gauss_hip.h by
// tests/test_xsusie_host.py: keeps the documented fields in step with the C ABI.
#include <cstdint>
#include <vector>

#include "gauss_hip.h"

// a, b: two imputation windows of one trait, one per study, filled as for gauss_impute_window (each its own populations or weights,
// measured SNPs and z1).  from_lead [Ma + Ua]: b's candidate index (measured first) of every candidate of a, -1 where b lacks the SNP
int xsusie_two_studies(gauss_ctx* ctx, gauss_window_desc a, gauss_window_desc b, const std::vector<int32_t>& from_lead,
                       std::vector<double>& pip, std::vector<int32_t>& set, std::vector<double>& V, std::vector<double>& purity)
{
  const int L = 10, K = 2, T = a.n_measured + a.n_unmeasured;
  if (K > GAUSS_XS_MAX || (int)from_lead.size() != T) return GAUSS_E_INVALID;
  std::vector<int32_t> kept(L);
  int32_t n_joint = 0;
  pip.assign((size_t)T, 0.0);  set.assign((size_t)T, -1);  V.assign((size_t)K * L, 0.0);  purity.assign((size_t)K * L, 0.0);
  gauss_window_desc w[2] = {a, b};
  for (gauss_window_desc& d : w) {                                    // the members of a group share their susie_* arguments
    d.susie_L = L;  d.susie_coverage = 0.95;  d.susie_prior_var = 25.0;  d.susie_tol = 1e-4;  d.susie_max_sweeps = 100;
    d.susie_min_abs_corr = 0.5;  d.susie_estimate_var = 1;
    d.xs_group = 1;                                                   // equal positive ids in one job: one group; the first window leads
  }
  w[1].xs_from_lead = from_lead.data();                               // NULL: the same index (equal M and U)
  w[0].out_susie_pip = pip.data();  w[0].out_susie_set = set.data();  w[0].out_susie_kept = kept.data();      // the joint fit, leader order
  w[0].out_xs_V = V.data();  w[0].out_xs_purity = purity.data();  w[0].out_xs_n = &n_joint;                    // per study [K][L]
  gauss_job* job = nullptr;
  int rc = gauss_job_create(ctx, w, K, 0, &job);                      // a group needs a job: gauss_impute_window refuses xs_group
  if (rc == GAUSS_OK) rc = gauss_job_run(job);
  if (rc == GAUSS_OK) rc = gauss_job_fetch(job);
  if (job) gauss_job_destroy(job);
  return rc;
  // every member's out_status carries GAUSS_ST_SUSIE_NOFIT when MakePosDef repaired ANY window of the group
}
