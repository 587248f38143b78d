// Colocalisation of the traits of one multi-causal fit (k_susie.hip): do two traits share a causal SNP in this window, or do they have
// two different ones in LD?  coloc's bf_bf (Wallace 2021) on the fit's per-effect Bayes factors, the imputed SNPs among the candidates.
// For fitted traits a < b, a kept effect la of a and a kept effect lb of b, with l1 = the final lbf row la of trait a, l2 = row lb of
// trait b, J = the candidates admissible in both fits, n = |J|:
//     S1 = sum_J e^l1_j,   S2 = sum_J e^l2_j,   S12 = sum_J e^(l1_j + l2_j)
//     lH0 = 0,   lH1 = log p1 + log S1,   lH2 = log p2 + log S2,   lH3 = log p1 + log p2 + log(S1 S2 - S12),   lH4 = log p12 + log S12
//     PP = softmax(lH);   hit = argmax_J (l1_j + l2_j) (ties: the smaller index);   hit_pp = e^(l1_hit + l2_hit) / S12
// Every sum is shifted by its maximum; S1 S2 - S12 is formed in logs, log S1 + log S2 + log1p(-exp(log S12 - log S1 - log S2)), and is
// -inf where the ratio is >= 1: with n = 1 the two logs are the same double and PP.H3 is an exact 0.
// One workgroup per (la, lb, pair, window); it leaves at once, NaN / -1 behind it, when either effect is not kept or n = 0.  The
// workgroup of (0, 0) writes the pair's n.  It reads what the launches before it have written (the kept flags of susie_kept_kernel,
// the lbf rows susie_set_kernel has kept, the admissibility flags) and writes its own entries only.  fp64, no atomics, every sum in a
// fixed order: per thread j ascending, then susie_block_sum's.  Compiled with -ffp-contract=off.
#include "k_susie_common.h"

namespace gauss {

__global__ __launch_bounds__(SUSIE_T) void coloc_kernel(const Prob* __restrict__ probs, const int* __restrict__ map, int max_L)
{
    __shared__ double s_red[SUSIE_NW];
    const Prob& pb = susie_prob(probs, map, blockIdx.z);
    const int tid = threadIdx.x;
    const int la = blockIdx.x / max_L, lb = blockIdx.x % max_L, pair = blockIdx.y;
    const int T = pb.M + pb.U, L = pb.susie_L, k = pb.susie_k;
    if (!pb.coloc || la >= L || lb >= L || pair >= (k + 1) * k / 2) return;
    // pair -> (a, b), a < b <= k, in the order (0, 1), (0, 2), .., (k - 1, k)
    int a = 0, left = pair;
    while (left >= k - a) { left -= k - a; a++; }
    const int b = a + 1 + left;
    const SusieWs o = susie_ws_of(pb);
    const SusieLayout q = susie_layout(T, L, pb.susie_am != 0);
    const SusieMoreLayout mq = susie_more_layout(T, L, pb.susie_am != 0, pb.susie_lbf != 0, k, true);
    const SusieTrait ta = susie_trait(pb, o, a), tb = susie_trait(pb, o, b);
    const size_t tld = (size_t)cs_tld(T), e = ((size_t)pair * L + la) * L + lb;
    const auto out = pb.out_susie_more;
    const auto adm_a = ta.st + o.adm, adm_b = tb.st + o.adm;
    double cnt = 0.0;
    for (int j = tid; j < T; j += SUSIE_T) cnt += adm_a[j] != 0.0 && adm_b[j] != 0.0 ? 1.0 : 0.0;
    const double n = susie_block_sum(cnt, s_red, tid);
    if (la == 0 && lb == 0 && tid == 0) out[mq.n + pair] = n;
    const bool kept = ta.out[q.kept + la] != 0.0 && tb.out[q.kept + lb] != 0.0;
    if (!kept || !(n > 0.0)) {
        if (tid == 0) {
            for (int h = 0; h < 5; h++) out[mq.pp + 5 * e + h] = __builtin_nan("");
            out[mq.hit + e] = -1.0; out[mq.hit_pp + e] = __builtin_nan("");
        }
        return;
    }
    const auto l1 = ta.st + o.keep + (size_t)la * tld, l2 = tb.st + o.keep + (size_t)lb * tld;
    // the three maxima; the candidate of the largest l1 + l2, the smaller index among equals
    const double ninf = -__builtin_inf();
    double m1 = ninf, m2 = ninf, m12 = ninf;
    int at = T;
    for (int j = tid; j < T; j += SUSIE_T)
        if (adm_a[j] != 0.0 && adm_b[j] != 0.0) {
            const double x = l1[j], y = l2[j], s = x + y;
            m1 = cs_max(m1, x); m2 = cs_max(m2, y);
            if (s > m12) { m12 = s; at = j; }
        }
    const double mine = m12;
    m1 = susie_block_max(m1, s_red, tid);
    m2 = susie_block_max(m2, s_red, tid);
    m12 = susie_block_max(m12, s_red, tid);
    // (indices are below 2^31: exact as doubles; a thread whose best is not the workgroup's stands back with -T)
    const double hit = -susie_block_max(mine == m12 && at < T ? -(double)at : -(double)T, s_red, tid);
    double s1 = 0.0, s2 = 0.0, s12 = 0.0;
    for (int j = tid; j < T; j += SUSIE_T)
        if (adm_a[j] != 0.0 && adm_b[j] != 0.0) {
            const double x = l1[j], y = l2[j];
            s1 += exp(x - m1); s2 += exp(y - m2); s12 += exp((x + y) - m12);
        }
    s1 = susie_block_sum(s1, s_red, tid);
    s2 = susie_block_sum(s2, s_red, tid);
    s12 = susie_block_sum(s12, s_red, tid);
    if (tid != 0) return;
    const double ls1 = m1 + log(s1), ls2 = m2 + log(s2), ls12 = m12 + log(s12);
    const double both = ls1 + ls2, ratio = ls12 - both;
    double lh[5];
    lh[0] = 0.0;
    lh[1] = log(pb.coloc_p1) + ls1;
    lh[2] = log(pb.coloc_p2) + ls2;
    lh[3] = ratio >= 0.0 ? ninf : (log(pb.coloc_p1) + log(pb.coloc_p2)) + (both + log1p(-exp(ratio)));
    lh[4] = log(pb.coloc_p12) + ls12;
    double top = lh[0];
    for (int h = 1; h < 5; h++) top = cs_max(top, lh[h]);
    double w[5], tot = 0.0;
    for (int h = 0; h < 5; h++) { w[h] = exp(lh[h] - top); tot += w[h]; }
    for (int h = 0; h < 5; h++) out[mq.pp + 5 * e + h] = w[h] / tot;
    out[mq.hit + e] = hit < (double)T ? hit : -1.0;
    out[mq.hit_pp + e] = 1.0 / s12;                          // e^(l1_hit + l2_hit - m12) = 1: the hit is where the maximum is
}

void launch_coloc(const Prob* d_probs, const int* d_susiemap, int n, int max_L, int max_k, hipStream_t s)
{
    if (n <= 0 || max_L <= 0 || max_k <= 0) return;
    hipLaunchKernelGGL(coloc_kernel, dim3(max_L * max_L, (max_k + 1) * max_k / 2, n), dim3(SUSIE_T), 0, s, d_probs, d_susiemap, max_L);
}

}  // namespace gauss
