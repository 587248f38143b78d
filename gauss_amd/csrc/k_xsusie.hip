// Joint fine-mapping across studies: the "sum of single effects" model of k_susie.hip fitted to K = 2 .. XS_MAX imputation windows of one
// job at once (a GROUP: one study each, each with its own ancestry weights, LD, scores and effect sizes), under the assumption that
// effect l sits at the SAME SNP in every study (the cross-population model of SuSiEx / MESuSiE).  The posterior over "which SNP",
// alpha_l, is shared; residuals, effect sizes and prior variances stay per study.
// Study k = 1 .. K (job order; study 1 is the LEADER) has the per-window quantities of k_susie.hip unchanged, in its own candidate
// order (measured first): B_k, C_k, z_k, W_k = B_k^-1 C_k^T, zhat_k, d_k, adm_k.  The joint candidates are the leader's candidates
// that are candidates of every study; Prob::xs_from_lead of study k maps leader candidate j to study k's index (-1: absent; null: the
// same index).  Joint admissible: every map entry >= 0 and adm_k true in every study.
// Fit (IBSS, Gauss-Seidel over l; every sum over candidates in LEADER order, studies ascending): V_lk = omega, bbar_lk = 0, f_k = 0;
//     r_k     = zhat_k - (f_k - R_k bbar_lk)                                  per study, own order
//     lbf_j   = sum_k susie_lbf(r_kj, d_kj, V_lk)                             joint candidates (every V_lk = 0: every lbf_j = 0)
//     alpha_l = softmax over the admissible joint candidates,   lse_l = max + log(sum / n_adm)
//     mu_lkj  = V_lk / (1 + V_lk d_kj) r_kj,   bbar_lk = alpha_l o mu_lk,   f_k and R_k bbar_lk as in k_susie.hip
//     estimate_var: V'_k = sum_j alpha_lj (mu_lkj^2 + s2_kj); lse(V'_1 .. V'_K) <= 0: every V_lk = 0 (joint, absorbing), else V_lk = V'_k
// delta, the stop rule, tol = 0 and max_sweeps are those of k_susie.hip.
// Launches (the launch boundary is the only synchronisation; what one launch writes no workgroup of that launch reads):
//   xsusie_ser_v_kernel   (sweep, l): grid = (slices of SUSIE_VR rows) x the group windows.  EVERY workgroup of EVERY member recomputes
//                         the joint single-effect update over the leader's candidates; it reads the peers' zhat, d, adm, f, R bbar_l and
//                         V through Prob::xs_peer and the maps.  The loop and the reduction order are the same in every workgroup, so
//                         every member holds bit-identical alpha, delta, lse and null-check decision.  Each workgroup then writes its
//                         rows of its own v_k; workgroup 0 of a member writes that member's own-order alpha, mu_k, lbf, next V_k, delta
//                         and its own done word.
//   susie_rb_kernel       (k_susie.hip) per member, as it is
//   susie_set_kernel, susie_rank_kernel (k_susie.hip) on the leader: membership on the joint lbf row in leader order, the top members
//   xsusie_purity_kernel  per (member, effect): the leader's top members mapped into the member's B / C / W
//   xsusie_kept_kernel    on the leader: purity_l = max over the studies (a set is pure if it is tight in at least one ancestry: this
//                         project's decision), kept, the per-effect outputs, the fit words, every study's V, purity and, where asked, mu
//   susie_fold_kernel     (k_susie.hip) on the leader: pip, set, set_pip from the shared alpha
// susie_w_kernel and susie_prep_kernel run per member.  fp64, no atomics; compiled with -ffp-contract=off.
#include "k_susie_common.h"

namespace gauss {

// The studies of a group as one (sweep, l) step reads them.  Every array is indexed by constants only (the loops over the studies are
// unrolled): it lives in registers.
struct XsView {
    int K, T_lead;
    GP(const double) zh[XS_MAX];
    GP(const double) dd[XS_MAX];
    GP(const double) adm[XS_MAX];
    GP(const double) f[XS_MAX];
    GP(const double) rb[XS_MAX];
    GP(const int) map[XS_MAX];
    int T[XS_MAX];
};

__device__ __forceinline__ int xs_clampK(int k) { return k < 2 ? 2 : (k > XS_MAX ? XS_MAX : k); }

__device__ __forceinline__ XsView xs_view(const Prob* probs, const Prob& pb, int l)
{
    XsView g;
    g.K = xs_clampK(pb.xs_n);
    const Prob& lead = probs[pb.xs_peer[0]];
    g.T_lead = lead.M + lead.U;
#pragma unroll
    for (int s = 0; s < XS_MAX; s++) {
        const Prob& q = probs[pb.xs_peer[s < g.K ? s : 0]];
        const SusieWs o = susie_ws_of(q);
        const auto ws = q.susie_ws;
        g.T[s] = q.M + q.U;
        g.zh[s] = ws + o.zhat; g.dd[s] = ws + o.d; g.adm[s] = ws + o.adm; g.f[s] = ws + o.f;
        g.rb[s] = ws + o.rb + (size_t)l * cs_tld(g.T[s]);
        g.map[s] = q.xs_from_lead;
    }
    return g;
}
// the studies' prior variances of effect l as sweep `sweep` reads them
__device__ __forceinline__ void xs_read_V(const Prob* probs, const Prob& pb, int K, int sweep, int l, double (&V)[XS_MAX])
{
#pragma unroll
    for (int s = 0; s < XS_MAX; s++) {
        const Prob& q = probs[pb.xs_peer[s < K ? s : 0]];
        V[s] = q.susie_ws[susie_ws_of(q).V + (size_t)(sweep & 1) * SUSIE_L + l];
    }
}
// leader candidate j in every study: idx[s] = study s's index of it.  false: it is no joint admissible candidate
__device__ __forceinline__ bool xs_joint(const XsView& g, int j, int (&idx)[XS_MAX])
{
    bool ok = true;
#pragma unroll
    for (int s = 0; s < XS_MAX; s++) {
        idx[s] = 0;
        if (s < g.K) {
            const int c = g.map[s] ? g.map[s][j] : j;
            const bool in = c >= 0 && c < g.T[s];           // (a validated map never leaves the window: plan time)
            idx[s] = in ? c : 0;
            ok = ok && in && g.adm[s][idx[s]] != 0.0;
        }
    }
    return ok;
}
// sum over the studies, ascending, of the single-effect log Bayes factors at an admissible joint candidate
__device__ __forceinline__ double xs_lbf(const XsView& g, const int (&idx)[XS_MAX], const double (&V)[XS_MAX])
{
    double lbf = 0.0;
#pragma unroll
    for (int s = 0; s < XS_MAX; s++)
        if (s < g.K) {
            const int c = idx[s];
            const double t = susie_lbf(g.zh[s][c] - (g.f[s][c] - g.rb[s][c]), g.dd[s][c], V[s]);
            lbf = s == 0 ? t : lbf + t;
        }
    return lbf;
}

// ---- one step of the joint fit ----
__global__ __launch_bounds__(SUSIE_T) void xsusie_ser_v_kernel(const Prob* __restrict__ probs, const int* __restrict__ map, int sweep, int l)
{
    __shared__ double s_b[SUSIE_CH], s_red[SUSIE_NW];
    const Prob& pb = susie_prob(probs, map, blockIdx.y);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = pb.M, U = pb.U, T = M + U, L = pb.susie_L;
    if (l >= L || sweep >= pb.susie_max_sweeps || (int)blockIdx.x * SUSIE_VR >= M) return;
    const SusieWs o = susie_ws_of(pb);
    const auto ws = pb.susie_ws;
    const auto ctl = ws + o.ctl;
    if (ctl[SUSIE_CTL_DONE] != 0.0) return;
    if (l == 0 && sweep > 0) {
        // every member holds the same delta: all of them leave at the same sweep, each by its own done word
        const double delta = ctl[SUSIE_CTL_DELTA + ((sweep - 1) & 1)];
        if (delta < pb.susie_tol) {
            if (blockIdx.x == 0 && tid == 0) { ctl[SUSIE_CTL_DONE] = 1.0; ctl[SUSIE_CTL_SWEEPS] = (double)sweep; ctl[SUSIE_CTL_LAST] = delta; }
            return;
        }
    }
    const XsView g = xs_view(probs, pb, l);
    const int K = g.K, TL = g.T_lead;
    double V[XS_MAX];
    xs_read_V(probs, pb, K, sweep, l, V);
    int idx[XS_MAX];
    // the joint single-effect update over the leader's candidates: max, then sum (j ascending per thread, then the fixed reduction)
    double mx = -__builtin_inf(), cnt = 0.0;
    for (int j = tid; j < TL; j += SUSIE_T)
        if (xs_joint(g, j, idx)) { mx = cs_max(mx, xs_lbf(g, idx, V)); cnt += 1.0; }
    mx = susie_block_max(mx, s_red, tid);
    const double n_adm = susie_block_sum(cnt, s_red, tid);
    double sum = 0.0;
    for (int j = tid; j < TL; j += SUSIE_T)
        if (xs_joint(g, j, idx)) sum += exp(xs_lbf(g, idx, V) - mx);
    sum = susie_block_sum(sum, s_red, tid);
    // this study's own values, in its own order
    const double Vown = ws[o.V + (size_t)(sweep & 1) * SUSIE_L + l];
    const size_t tld = (size_t)cs_tld(T);
    const auto zh = ws + o.zhat, dd = ws + o.d, f = ws + o.f, rb = ws + o.rb + (size_t)l * tld;
    const auto to_lead = pb.xs_to_lead;
    // alpha_j of own candidate c (0: no joint admissible candidate)
    auto alpha_of = [&](int c, double& lbf) -> double {
        const int j = to_lead ? to_lead[c] : c;
        if (j < 0 || j >= TL) return 0.0;
        int id[XS_MAX];
        if (!xs_joint(g, j, id)) return 0.0;
        lbf = xs_lbf(g, id, V);
        return exp(lbf - mx) / sum;
    };
    auto bbar = [&](int c) -> double {
        double lbf = 0.0;
        const double a = alpha_of(c, lbf);
        if (a == 0.0) return 0.0;
        return a * (Vown / (1.0 + Vown * dd[c]) * (zh[c] - (f[c] - rb[c])));
    };
    // this workgroup's rows of v_k = bbar_meas + W_k bbar_unmeas, as susie_ser_v_kernel forms them
    const int i0 = blockIdx.x * SUSIE_VR + 2 * wave;
    double acc0 = 0.0, acc1 = 0.0;
    if (!pb.susie_measured_only && U > 0) {
        const int uld = susie_uld(U);
        const auto W0 = pb.susie_ws + o.W + (size_t)min(i0, M - 1) * uld, W1 = pb.susie_ws + o.W + (size_t)min(i0 + 1, M - 1) * uld;
        for (int c0 = 0; c0 < U; c0 += SUSIE_CH) {
            const int n = min(SUSIE_CH, U - c0);
            __syncthreads();                                // (the chunk before has been read)
            for (int k = tid; k < n; k += SUSIE_T) s_b[k] = bbar(M + c0 + k);
            __syncthreads();
            for (int k = lane; k < n; k += 64) {
                const double b = s_b[k];
                acc0 += W0[c0 + k] * b;
                acc1 += W1[c0 + k] * b;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { acc0 += __shfl_xor(acc0, off, 64); acc1 += __shfl_xor(acc1, off, 64); }
    }
    if (lane == 0) {
        const auto v = ws + o.v;
        if (i0 < M) v[i0] = bbar(i0) + acc0;
        if (i0 + 1 < M) v[i0 + 1] = bbar(i0 + 1) + acc1;
    }
    if (blockIdx.x != 0) return;
    // workgroup 0 of the member.  Every study's new variance, in leader order: the same sums in every member
    double vnew[XS_MAX];
#pragma unroll
    for (int s = 0; s < XS_MAX; s++) vnew[s] = 0.0;
    for (int j = tid; j < TL; j += SUSIE_T)
        if (xs_joint(g, j, idx)) {
            const double a = exp(xs_lbf(g, idx, V) - mx) / sum;
#pragma unroll
            for (int s = 0; s < XS_MAX; s++)
                if (s < K) {
                    const int c = idx[s];
                    const double s2 = V[s] / (1.0 + V[s] * g.dd[s][c]), m = s2 * (g.zh[s][c] - (g.f[s][c] - g.rb[s][c]));
                    vnew[s] += a * (m * m + s2);
                }
        }
    bool any = false;
#pragma unroll
    for (int s = 0; s < XS_MAX; s++)
        if (s < K) { vnew[s] = susie_block_sum(vnew[s], s_red, tid); any = any || V[s] != 0.0; }
    double vnext = Vown;
    if (pb.susie_estimate_var && any) {
        // the joint null check of the new variances: lse(V'_1 .. V'_K) <= 0 says that no effect beats one, in any study
        double mx2 = -__builtin_inf();
        for (int j = tid; j < TL; j += SUSIE_T)
            if (xs_joint(g, j, idx)) mx2 = cs_max(mx2, xs_lbf(g, idx, vnew));
        mx2 = susie_block_max(mx2, s_red, tid);
        double sum2 = 0.0;
        for (int j = tid; j < TL; j += SUSIE_T)
            if (xs_joint(g, j, idx)) sum2 += exp(xs_lbf(g, idx, vnew) - mx2);
        sum2 = susie_block_sum(sum2, s_red, tid);
        const double lse2 = mx2 + log(sum2 / n_adm);
        double own = 0.0;
#pragma unroll
        for (int s = 0; s < XS_MAX; s++) own = s == pb.xs_pos ? vnew[s] : own;
        vnext = lse2 <= 0.0 || n_adm == 0.0 ? 0.0 : own;                    // (a NaN keeps V': nothing is decided on it)
    }
    // the member's alpha, mu_k and lbf in its own order, and the running delta (the same set of values in every member: the joint
    // candidates once each, zeros elsewhere -- a maximum does not depend on their order)
    const auto al = ws + o.alpha + (size_t)l * tld, mu = ws + o.mu + (size_t)l * tld, lb = ws + o.lbf + (size_t)l * tld;
    double delta = 0.0;
    for (int c = tid; c < T; c += SUSIE_T) {
        double lbf = -__builtin_inf(), m = 0.0;             // (alpha_of leaves lbf alone where c is no joint admissible candidate)
        const double a = alpha_of(c, lbf);
        if (lbf != -__builtin_inf()) m = Vown / (1.0 + Vown * dd[c]) * (zh[c] - (f[c] - rb[c]));
        delta = cs_max(delta, fabs(a - al[c]));
        al[c] = a; mu[c] = m; lb[c] = lbf;
    }
    delta = susie_block_max(delta, s_red, tid);
    if (tid == 0) {
        ws[o.V + (size_t)((sweep + 1) & 1) * SUSIE_L + l] = vnext;
        ws[o.lse + l] = n_adm > 0.0 ? mx + log(sum / n_adm) : __builtin_nan("");
        const int slot = SUSIE_CTL_DELTA + (sweep & 1);
        ctl[slot] = l == 0 ? delta : cs_max(ctl[slot], delta);
    }
}

// ---- sets ----
__global__ __launch_bounds__(SUSIE_T) void xsusie_purity_kernel(const Prob* __restrict__ probs, const int* __restrict__ map)
{
    __shared__ double s_min[SUSIE_NW];
    __shared__ int s_top[SUSIE_P];
    const Prob& pb = susie_prob(probs, map, blockIdx.z);
    const Prob& lead = probs[pb.xs_peer[0]];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.x, l = blockIdx.y;
    const int M = pb.M, U = pb.U, T = M + U, L = pb.susie_L, ld = pb.Mld, TL = lead.M + lead.U;
    if (l >= L) return;
    const SusieWs o = susie_ws_of(pb), ol = susie_ws_of(lead);
    const auto ws = pb.susie_ws;
    const auto wl = lead.susie_ws;
    const double np = wl[ol.ntop + l];
    const int P = __builtin_amdgcn_readfirstlane(np >= 0.0 && np <= (double)SUSIE_P ? (int)np : 0);
    const auto top = (GP(const int))(wl + ol.top) + l * SUSIE_P;
    const auto from = pb.xs_from_lead;
    const int lim = pb.susie_measured_only ? M : T;         // (a fit of the measured SNPs alone has no W to read)
    for (int k = tid; k < SUSIE_P; k += SUSIE_T) {
        int c = k < P ? top[k] : 0;
        c = c >= 0 && c < TL ? c : 0;                       // (whatever a group that is not fitted has left there: nothing is indexed outside)
        if (from) c = from[c];
        s_top[k] = c >= 0 && c < lim ? c : 0;
    }
    __syncthreads();
    const auto dd = ws + o.d;
    const int uld = susie_uld(U);
    double mn = __builtin_inf();
    int q = 0;
    for (int a = 0; a < P; a++)
        for (int b = a + 1; b < P; b++, q++) {
            if (q % (SUSIE_PG * SUSIE_NW) != g * SUSIE_NW + wave) continue;
            const int ca = min(s_top[a], s_top[b]), cb = max(s_top[a], s_top[b]);
            double r;
            if (cb < M) r = pb.A[(size_t)ca * ld + cb];
            else if (ca < M) r = pb.B21[(size_t)(cb - M) * ld + ca];
            else {
                // c_u . W_v over the measured SNPs, a lane the rows lane, + 64, ...
                const auto cu = pb.B21 + (size_t)(ca - M) * ld;
                const auto wv = pb.susie_ws + o.W + (cb - M);
                double acc = 0.0;
                for (int m = lane; m < M; m += 64) acc += cu[m] * wv[(size_t)m * uld];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
                r = acc;
            }
            const double pur = fabs(r) / sqrt(dd[ca] * dd[cb]);
            mn = pur < mn ? pur : mn;
        }
    if (lane == 0) s_min[wave] = mn;
    __syncthreads();
    if (tid == 0) {
        double t = s_min[0];
#pragma unroll
        for (int w = 1; w < SUSIE_NW; w++) t = s_min[w] < t ? s_min[w] : t;
        ws[o.part + (size_t)l * SUSIE_PG + g] = t;
    }
}

// grid = (leaders, 1 + XS_MAX): row 0 the sets and the fit words, row 1 + k study k's mu in leader order where it is asked
__global__ __launch_bounds__(SUSIE_T) void xsusie_kept_kernel(const Prob* __restrict__ probs, const int* __restrict__ map)
{
    __shared__ double s_red[SUSIE_NW];
    __shared__ int s_kept[SUSIE_L];
    const Prob& pb = susie_prob(probs, map, blockIdx.x);
    const int tid = threadIdx.x;
    const int T = pb.M + pb.U, L = pb.susie_L, K = xs_clampK(pb.xs_n);
    const SusieWs o = susie_ws_of(pb);
    const SusieLayout q = susie_layout(T, L, pb.susie_am != 0);
    const XsLayout x = xs_layout(K, L, T, pb.xs_mu != 0);
    const auto ws = pb.susie_ws;
    const auto out = pb.out_susie;
    const auto xo = pb.out_xs;
    const size_t tld = (size_t)cs_tld(T);
    if (blockIdx.y > 0) {
        const int k = (int)blockIdx.y - 1;
        if (!pb.xs_mu || k >= K) return;
        const Prob& qk = probs[pb.xs_peer[k]];
        const int Tk = qk.M + qk.U;
        const SusieWs ok = susie_ws_of(qk);
        const auto from = qk.xs_from_lead;
        for (size_t e = tid; e < (size_t)L * T; e += SUSIE_T) {
            const int l = (int)(e / T), j = (int)(e % T);
            const int c = from ? from[j] : j;
            xo[x.mu + ((size_t)k * L + l) * T + j] = c >= 0 && c < Tk ? qk.susie_ws[ok.mu + (size_t)l * cs_tld(Tk) + c] : 0.0;
        }
        return;
    }
    const int sweeps = susie_sweeps_of(pb, ws + o.ctl);
    // the joint admissible candidates
    const XsView g = xs_view(probs, pb, 0);
    int idx[XS_MAX];
    double cnt = 0.0;
    for (int j = tid; j < T; j += SUSIE_T) cnt += xs_joint(g, j, idx) ? 1.0 : 0.0;
    cnt = susie_block_sum(cnt, s_red, tid);
    for (int l = 0; l < L; l++) {
        const double np = ws[o.ntop + l];
        // every study's V of the last sweep's update and its purity of the leader's top members; the set's purity is their maximum
        double purity = np >= 2.0 ? -__builtin_inf() : (np == 1.0 ? 1.0 : __builtin_nan(""));
        bool any = false;
        double V1 = 0.0;
#pragma unroll
        for (int k = 0; k < XS_MAX; k++)
            if (k < K) {
                const Prob& qk = probs[pb.xs_peer[k]];
                const SusieWs ok = susie_ws_of(qk);
                const double Vk = qk.susie_ws[ok.V + (size_t)(sweeps & 1) * SUSIE_L + l];
                double pk = np >= 2.0 ? __builtin_inf() : purity;
                if (np >= 2.0)
                    for (int gi = 0; gi < SUSIE_PG; gi++) { const double t = qk.susie_ws[ok.part + (size_t)l * SUSIE_PG + gi]; pk = t < pk ? t : pk; }
                if (np >= 2.0) purity = pk > purity ? pk : purity;
                any = any || Vk > 0.0;
                if (k == 0) V1 = Vk;
                if (tid == 0) { xo[x.V + (size_t)k * L + l] = Vk; xo[x.purity + (size_t)k * L + l] = pk; }
            }
        bool kept = any && purity >= pb.susie_min_abs_corr;
        // no kept set in front of it has the same members
        for (int k = 0; k < l && kept; k++) {
            if (!s_kept[k] || out[q.size + k] != out[q.size + l]) continue;      // (s_kept[k]: written behind a barrier of iteration k)
            double diff = 0.0;
            for (int i = tid; i < T; i += SUSIE_T) diff += pb.susie_mem[(size_t)k * tld + i] != pb.susie_mem[(size_t)l * tld + i] ? 1.0 : 0.0;
            diff = susie_block_sum(diff, s_red, tid);
            if (diff == 0.0) kept = false;
        }
        __syncthreads();
        if (tid == 0) {
            s_kept[l] = kept ? 1 : 0;
            out[q.V + l] = V1; out[q.lse + l] = ws[o.lse + l]; out[q.purity + l] = purity; out[q.kept + l] = kept ? 1.0 : 0.0;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const auto ctl = ws + o.ctl;
        const bool done = ctl[SUSIE_CTL_DONE] != 0.0;
        const double delta = done ? ctl[SUSIE_CTL_LAST] : ctl[SUSIE_CTL_DELTA + ((sweeps - 1) & 1)];
        out[q.fit] = (double)sweeps; out[q.fit + 1] = delta;
        out[q.fit + 2] = delta < pb.susie_tol ? 0.0 : 1.0;      // the sweeps ran out first
        out[q.fit + 3] = 0.0;
        xo[x.n] = cnt;
    }
}

void launch_xsusie(const Prob* d_probs, const int* d_xsmap, int n, const int* d_xsleadmap, int n_lead, int max_M, int max_T, int max_L,
                   int max_sweeps, hipStream_t s)
{
    if (n <= 0 || n_lead <= 0 || max_T <= 0) return;
    launch_susie_prep(d_probs, d_xsmap, n, s);
    const dim3 gv((max_M + SUSIE_VR - 1) / SUSIE_VR, n, 1);
    for (int sweep = 0; sweep < max_sweeps; sweep++)
        for (int l = 0; l < max_L; l++) {
            hipLaunchKernelGGL(xsusie_ser_v_kernel, gv, dim3(SUSIE_T), 0, s, d_probs, d_xsmap, sweep, l);
            launch_susie_rb(d_probs, d_xsmap, n, max_T, sweep, l, s);
        }
    launch_susie_sets(d_probs, d_xsleadmap, n_lead, max_L, s);
    hipLaunchKernelGGL(xsusie_purity_kernel, dim3(SUSIE_PG, max_L, n), dim3(SUSIE_T), 0, s, d_probs, d_xsmap);
    hipLaunchKernelGGL(xsusie_kept_kernel, dim3(n_lead, 1 + XS_MAX, 1), dim3(SUSIE_T), 0, s, d_probs, d_xsleadmap);
    launch_susie_fold(d_probs, d_xsleadmap, n_lead, max_T, s);
}

}  // namespace gauss
