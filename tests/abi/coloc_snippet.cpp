// The Rcpp-side code of INTEGRATION.md section 5m5 (every trait of a window in one fit, and the colocalisation of their signals),
// compiled against include/gauss_hip.h by tests/test_coloc_host.py: keeps the documented fields in step with the C ABI.
#include <cstdint>
#include <vector>

#include "gauss_hip.h"

// z_more [T x M] row-major: the further traits' Z-scores at the window's measured SNPs; the first k of them are fitted beside z1
int coloc_window(gauss_ctx* ctx, gauss_window_desc w, int M, int U, int T, int k, const std::vector<double>& z_more,
                 std::vector<double>& pp, std::vector<int32_t>& hit, std::vector<double>& hit_pp, std::vector<int32_t>& kept_more)
{
  const int L = 10, pairs = (k + 1) * k / 2;
  if (k > GAUSS_SUSIE_TRAITS_MORE_MAX || k > T) return GAUSS_E_INVALID;
  std::vector<double> out_z_more((size_t)T * U), pip_more((size_t)k * (M + U));
  std::vector<int32_t> kept(L), status_more(k), n(pairs);
  pp.assign((size_t)pairs * L * L * 5, 0.0);  hit.assign((size_t)pairs * L * L, -1);  hit_pp.assign((size_t)pairs * L * L, 0.0);
  kept_more.assign((size_t)k * L, 0);
  w.n_traits_more = T;  w.z_more = z_more.data();  w.out_z_more = out_z_more.data();      // the further traits, imputed as before
  w.susie_L = L;  w.susie_coverage = 0.95;  w.susie_prior_var = 25.0;  w.susie_tol = 1e-4;  w.susie_max_sweeps = 100;
  w.susie_min_abs_corr = 0.5;  w.susie_estimate_var = 1;
  w.out_susie_kept = kept.data();
  w.coloc_traits_more = k;                                            // ... and fitted with z1, in the same launches
  w.out_coloc_more_pip = pip_more.data();  w.out_coloc_more_kept = kept_more.data();  w.out_coloc_more_status = status_more.data();
  w.coloc_p1 = 1e-4;  w.coloc_p2 = 1e-4;  w.coloc_p12 = 1e-5;         // coloc's defaults; all zero: no pairs
  w.out_coloc_pp = pp.data();  w.out_coloc_hit = hit.data();  w.out_coloc_hit_pp = hit_pp.data();  w.out_coloc_n = n.data();
  return gauss_impute_window(ctx, &w);
  // pair q of (0, 1), (0, 2), .., (k - 1, k), trait 0 being z1; effects la of its first and lb of its second trait:
  // pp[((q L + la) L + lb) 5 + h] = P(H_h), NaN unless both effects are kept; hit[..] = the candidate (c < M measured, M + u imputed)
  // most likely shared, hit_pp[..] its share of H4.  status_more[t]: GAUSS_ST_SUSIE_NOCONV / GAUSS_ST_SUSIE_NOFIT of further trait t.
}
