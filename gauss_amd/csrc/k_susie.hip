// Multi-causal fine-mapping of a window: the "sum of single effects" model fitted to the measured z (SuSiE-RSS, Zou et al. 2022), with
// the unmeasured SNPs of the window as candidates beside the measured ones.  Notation: B = B11 [M x M] (A[0], lambda on the diagonal),
// C = B21 [U x M], z = z1, A = [B | C^T] [M x T], T = M + U; candidates are indexed measured first, then unmeasured.
//     R = A^T B^-1 A [T x T, rank M],   zhat = A^T B^-1 z = [z ; m]   (m_u = out_z[u] sqrt(out_info[u]), the conditional mean)
//     d_j = R_jj = B_jj (measured), out_info[u] (unmeasured)
// Model: z ~ N(A sum_l b_l, B), l = 1 .. L, b_l with one non-zero entry at a candidate drawn uniformly from the admissible ones, its
// value ~ N(0, V_l).  Admissible: zhat_j finite, d_j finite and > 0, measured or !measured_only, and no unmeasured SNP when z1 holds a
// non-finite value.  An inadmissible candidate has alpha = mu = 0 and enters no sum.
// Fit (IBSS, Gauss-Seidel over l): bbar_l = 0, V_l = omega, f = 0; one sweep, l = 1 .. L in order:
//     r     = zhat - (f - R bbar_l)
//     lbf_j = ( r_j^2 V_l / (1 + V_l d_j) - log1p(V_l d_j) ) / 2                      (V_l = 0: lbf_j = 0)
//     lse_l = max + log( sum_j exp(lbf_j - max) / n_adm ),   alpha_lj = exp(lbf_j - max) / sum
//     s2_j  = V_l / (1 + V_l d_j),   mu_lj = s2_j r_j,   bbar_l = alpha_l o mu_l,   f = (f - R bbar_l_old) + R bbar_l_new
//     estimate_var: V' = sum_j alpha_lj (mu_lj^2 + s2_j); V' = 0 if lse(V') <= 0; V_l = V' from the next sweep on (V_l = 0 is absorbing)
// After a sweep delta = max_lj |alpha_lj - alpha_lj(sweep before)|; the fit stops when delta < tol or after max_sweeps sweeps.
// Nothing T x T is formed: with W = B^-1 C^T = X^T (X C^T) [M x U] (X = L^-1, the rows the fused solve leaves in V),
//     v = bbar_meas + W bbar_unmeas,    R bbar = A^T v = [B v ; C v]
// two dependent matrix-vector products per (sweep, l).
//
// Launches (the launch boundary is the only synchronisation between workgroups: no workgroup waits for another, nothing spins):
//   susie_w_kernel        pass 0: Y = X C^T, pass 1: W = X^T Y, by (64-row block, 64 unmeasured SNPs) on the traits kernels' MFMA chain
//                         (k_traits_common.h); where the traits weights run.  Not launched for measured_only windows.
//   susie_prep_kernel     zhat, d, the admissibility flags; the state zeroed, V = omega
//   susie_ser_v_kernel    (sweep, l): grid = (slices of SUSIE_VR rows of M) x windows.  EVERY workgroup recomputes the single-effect
//                         update of effect l over all T candidates (max, sum: a few thousand exp, identical bits in every workgroup),
//                         then writes its rows of v; the unmeasured candidates' bbar pass through LDS SUSIE_CH at a time.  Workgroup 0
//                         also writes alpha_l, mu_l, lbf_l, lse_l, the next V_l and the running delta.  At l = 0 every workgroup reads
//                         the delta of the sweep before: below tol, the window is done (workgroup 0 sets the word) and leaves.
//   susie_rb_kernel       (sweep, l): grid = (slices of SUSIE_RR candidates) x windows: R bbar_l = [B v ; C v] and f for its rows.
//   All max_sweeps x L x 2 launches are queued up front; a window whose done word is set, or that has fewer effects or sweeps than
//   the job's largest, leaves at once.  V_l and delta are kept by sweep parity: what one launch writes no workgroup of it reads.
//   susie_set_kernel      one workgroup per (effect, window): cs_set_row (k_cs_common.h) on the final lbf row: membership.
//   susie_rank_kernel     one workgroup per (effect, window): the P = min(size, SUSIE_P) members of largest alpha (ties: smaller index)
//   susie_purity_kernel   SUSIE_PG workgroups per (effect, window), one wave per pair: min |R_ij| / sqrt(d_i d_j), R_ij = B_ij, C_ui
//                         or c_u . W_v
//   susie_kept_kernel     one workgroup per window: purity, kept (V_l > 0, purity >= min_abs_corr, no kept l' < l with the same members),
//                         the per-effect outputs, sweeps / delta / the no-convergence flag
//   susie_fold_kernel     one thread per candidate: pip = 1 - prod_{V_l > 0} (1 - alpha_lj), set, set_pip over the kept sets
//   coloc_kernel          (k_coloc.hip) behind susie_kept_kernel where a window asks: the pairs of kept effects of two fitted traits
// Further traits (Prob::susie_k of the window's further Z-score vectors, k_traits.hip) are fitted in the same launches: the trait is
// blockIdx.z of prep, ser_v, rb, set, rank, kept and fold, and rides with the effect in blockIdx.y of purity.  B, C, W and Y are the
// window's; a trait reads its own scores (susie_trait, k_susie_common.h) and keeps its own state, done word included, so every trait
// leaves the step launches at its own sweep.  Trait 0's pointers, sums and bits are those of a fit of one trait.
// fp64, no atomics, every sum in a fixed order.  Compiled with -ffp-contract=off like the other fp64 tails.
#include "k_traits_common.h"
#include "k_susie_common.h"

namespace gauss {

static_assert(SUSIE_VR == 2 * SUSIE_NW && SUSIE_RR == 2 * SUSIE_NW, "two rows a wave");
static_assert(SUSIE_L <= SLCT_K, "cs_set_row's workspace geometry");

// ---- W = X^T (X C^T) ----
__global__ __launch_bounds__(256) void susie_w_kernel(const Prob* __restrict__ probs, const int* __restrict__ map, int pass)
{
    __shared__ __attribute__((aligned(16))) double TA[NB * TLA];
    __shared__ __attribute__((aligned(16))) double TB[TK * TLB];
    const Prob& pb = susie_prob(probs, map, blockIdx.z);
    const int blk = blockIdx.x, cg = blockIdx.y;
    const int M = pb.M, U = pb.U, ld = pb.Mld;
    if (pb.susie_measured_only || blk >= pb.nblk || cg * NB >= U) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int uld = susie_uld(U);
    const SusieWs o = susie_ws_of(pb);
    const auto Y = pb.susie_ws + o.Y, W = pb.susie_ws + o.W;
    f64x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; n++) acc[n] = f64x4{0.0, 0.0, 0.0, 0.0};
    if (pass == 0) {
        // Y[64 blk + r][u] = sum over g <= k of X[k][g] C[u][g]: traits_weights_kernel's pass 0 with column u of C^T as the trait
        const int n_stage = min(2 * (blk + 1), (M + TK - 1) / TK);
        for (int st = 0; st < n_stage; st++) {
            const int g0 = st * TK;
            const auto xp = pb.V + (size_t)(g0 >> 6) * ld * NR + (g0 & 63);
            for (int e = tid; e < NB * TK; e += 256) {
                const int r = e / TK, c = e % TK;
                const int k = blk * NB + r, g = g0 + c;
                const double x = xp[(size_t)k * NR + c];           // in range whatever it holds: panel <= blk < npi, k < Mld, column < NR
                TA[r * TLA + c] = (g <= k && k < M) ? x : 0.0;
            }
            for (int e = tid; e < TK * NB; e += 256) {
                const int r = e % TK, c = e / TK;                  // r fastest: a row of B21 is contiguous over g
                const int g = g0 + r, u = cg * NB + c;
                const double b = pb.B21[(size_t)min(u, U - 1) * ld + g];      // g < Mld
                TB[r * TLB + c] = (u < U && g < M) ? b : 0.0;
            }
            __syncthreads();
            traits_mma(acc, TA, TB, wave, lane, 4);
            __syncthreads();
        }
    } else {
        traits_xt_y(acc, pb.V, Y + cg * NB, blk, M, ld, uld, NB, TA, TB, tid, wave, lane);
    }
    const auto out = pass == 0 ? Y : W;
#pragma unroll
    for (int n = 0; n < 4; n++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = blk * NB + 16 * wave + (lane >> 4) + 4 * r;     // the f64 shape's C/D map; row < Mld, column < uld
            out[(size_t)row * uld + cg * NB + 16 * n + (lane & 15)] = acc[n][r];
        }
}

// ---- the state ----
__global__ __launch_bounds__(SUSIE_T) void susie_prep_kernel(const Prob* __restrict__ probs, const int* __restrict__ map)
{
    __shared__ double s_red[SUSIE_NW];
    const Prob& pb = susie_prob(probs, map, blockIdx.y);
    const int tid = threadIdx.x;
    const int M = pb.M, U = pb.U, T = M + U, ld = pb.Mld;
    if ((int)blockIdx.z > pb.susie_k) return;
    const SusieWs o = susie_ws_of(pb);
    const SusieTrait tr = susie_trait(pb, o, blockIdx.z);
    const auto ws = tr.st;
    const size_t stride = (size_t)gridDim.x * SUSIE_T, first = (size_t)blockIdx.x * SUSIE_T + tid;
    // a non-finite score of the trait anywhere: no unmeasured SNP is admissible (every workgroup looks for itself)
    double bad = 0.0;
    for (int i = tid; i < M; i += SUSIE_T) bad += isfinite(tr.z[(size_t)i * tr.zs]) ? 0.0 : 1.0;
    bad = susie_block_sum(bad, s_red, tid);
    for (size_t e = o.state + first; e < o.keep; e += stride) {
        double x = 0.0;
        if (e >= o.V && e < o.V + 2 * SUSIE_L) x = pb.susie_prior_var;
        if (e == o.ctl + SUSIE_CTL_ZNAN) x = bad;
        ws[e] = x;
    }
    for (size_t j = first; j < (size_t)T; j += stride) {
        double zh, d;
        bool adm;
        if (j < (size_t)M) {
            zh = tr.z[j * tr.zs]; d = pb.A[j * ld + j];
            adm = true;
        } else {
            const double zu = tr.zu[j - M], info = pb.out_info[j - M];
            zh = zu * sqrt(info); d = info;
            adm = !pb.susie_measured_only && bad == 0.0;
        }
        adm = adm && isfinite(zh) && isfinite(d) && d > 0.0;
        ws[o.zhat + j] = zh; ws[o.d + j] = d; ws[o.adm + j] = adm ? 1.0 : 0.0;
    }
}

// ---- one step of the fit ----
__global__ __launch_bounds__(SUSIE_T) void susie_ser_v_kernel(const Prob* __restrict__ probs, const int* __restrict__ map, int sweep, int l)
{
    __shared__ double s_b[SUSIE_CH], s_red[SUSIE_NW];
    const Prob& pb = susie_prob(probs, map, blockIdx.y);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = pb.M, U = pb.U, T = M + U, L = pb.susie_L;
    if (l >= L || sweep >= pb.susie_max_sweeps || (int)blockIdx.x * SUSIE_VR >= M || (int)blockIdx.z > pb.susie_k) return;
    const SusieWs o = susie_ws_of(pb);
    const auto ws = pb.susie_ws + (size_t)blockIdx.z * o.trait;      // the trait's state
    const auto ctl = ws + o.ctl;
    if (ctl[SUSIE_CTL_DONE] != 0.0) return;
    if (l == 0 && sweep > 0) {
        // the sweep before has moved no alpha by tol: converged.  Every workgroup of this launch decides the same from what the launches
        // before have written; workgroup 0 leaves the word for the launches that follow
        const double delta = ctl[SUSIE_CTL_DELTA + ((sweep - 1) & 1)];
        if (delta < pb.susie_tol) {
            if (blockIdx.x == 0 && tid == 0) { ctl[SUSIE_CTL_DONE] = 1.0; ctl[SUSIE_CTL_SWEEPS] = (double)sweep; ctl[SUSIE_CTL_LAST] = delta; }
            return;
        }
    }
    const size_t tld = (size_t)cs_tld(T);
    const double V = ws[o.V + (size_t)(sweep & 1) * SUSIE_L + l];
    const auto zh = ws + o.zhat, dd = ws + o.d, adm = ws + o.adm, f = ws + o.f, rb = ws + o.rb + (size_t)l * tld;
    // the single-effect update of effect l over every candidate: max, then sum (j ascending per thread, then the fixed reduction)
    double mx = -__builtin_inf(), cnt = 0.0;
    for (int j = tid; j < T; j += SUSIE_T)
        if (adm[j] != 0.0) { mx = cs_max(mx, susie_lbf(zh[j] - (f[j] - rb[j]), dd[j], V)); cnt += 1.0; }
    mx = susie_block_max(mx, s_red, tid);
    const double n_adm = susie_block_sum(cnt, s_red, tid);
    double sum = 0.0;
    for (int j = tid; j < T; j += SUSIE_T)
        if (adm[j] != 0.0) sum += exp(susie_lbf(zh[j] - (f[j] - rb[j]), dd[j], V) - mx);
    sum = susie_block_sum(sum, s_red, tid);
    // (no admissible candidate at all -- every z1 non-finite: mx = -inf and sum = 0 are never used, every alpha, mu and bbar below is an
    // exact zero, v = 0, and lse_l is NaN as the definition's log(0 / 0) is)
    // bbar_j = alpha_j mu_j
    auto bbar = [&](int j) -> double {
        if (adm[j] == 0.0) return 0.0;
        const double r = zh[j] - (f[j] - rb[j]), d = dd[j];
        return exp(susie_lbf(r, d, V) - mx) / sum * (V / (1.0 + V * d) * r);
    };
    // this workgroup's rows of v = bbar_meas + W bbar_unmeas: wave w the rows 2 w, 2 w + 1 of the slice, a lane the columns lane, + 64, ...
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
    // workgroup 0: the effect's alpha, mu and lbf, the running delta, lse and the next V
    const auto al = ws + o.alpha + (size_t)l * tld, mu = ws + o.mu + (size_t)l * tld, lb = ws + o.lbf + (size_t)l * tld;
    double delta = 0.0, vnew = 0.0;
    for (int j = tid; j < T; j += SUSIE_T) {
        double a = 0.0, m = 0.0, lbf = -__builtin_inf();
        if (adm[j] != 0.0) {
            const double r = zh[j] - (f[j] - rb[j]), d = dd[j], s2 = V / (1.0 + V * d);
            lbf = susie_lbf(r, d, V);
            a = exp(lbf - mx) / sum;
            m = s2 * r;
            vnew += a * (m * m + s2);
        }
        delta = cs_max(delta, fabs(a - al[j]));
        al[j] = a; mu[j] = m; lb[j] = lbf;
    }
    delta = susie_block_max(delta, s_red, tid);
    vnew = susie_block_sum(vnew, s_red, tid);
    double vnext = V;
    if (pb.susie_estimate_var && V != 0.0) {
        // the null check of the new variance: lse(V') <= 0 says that no effect beats one
        double mx2 = -__builtin_inf();
        for (int j = tid; j < T; j += SUSIE_T)
            if (adm[j] != 0.0) mx2 = cs_max(mx2, susie_lbf(zh[j] - (f[j] - rb[j]), dd[j], vnew));
        mx2 = susie_block_max(mx2, s_red, tid);
        double sum2 = 0.0;
        for (int j = tid; j < T; j += SUSIE_T)
            if (adm[j] != 0.0) sum2 += exp(susie_lbf(zh[j] - (f[j] - rb[j]), dd[j], vnew) - mx2);
        sum2 = susie_block_sum(sum2, s_red, tid);
        const double lse2 = mx2 + log(sum2 / n_adm);
        vnext = lse2 <= 0.0 || n_adm == 0.0 ? 0.0 : vnew;                   // (a NaN keeps V': nothing is decided on it)
    }
    if (tid == 0) {
        ws[o.V + (size_t)((sweep + 1) & 1) * SUSIE_L + l] = vnext;
        ws[o.lse + l] = n_adm > 0.0 ? mx + log(sum / n_adm) : __builtin_nan("");
        const int slot = SUSIE_CTL_DELTA + (sweep & 1);
        ctl[slot] = l == 0 ? delta : cs_max(ctl[slot], delta);
    }
}

__global__ __launch_bounds__(SUSIE_T) void susie_rb_kernel(const Prob* __restrict__ probs, const int* __restrict__ map, int sweep, int l)
{
    const Prob& pb = susie_prob(probs, map, blockIdx.y);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = pb.M, T = M + pb.U, L = pb.susie_L, ld = pb.Mld;
    const int rows = pb.susie_measured_only ? M : T;        // (an inadmissible candidate's row is never read)
    if (l >= L || sweep >= pb.susie_max_sweeps || (int)blockIdx.x * SUSIE_RR >= rows || (int)blockIdx.z > pb.susie_k) return;
    const SusieWs o = susie_ws_of(pb);
    const auto ws = pb.susie_ws + (size_t)blockIdx.z * o.trait;      // the trait's state
    if (ws[o.ctl + SUSIE_CTL_DONE] != 0.0) return;
    const auto v = ws + o.v, f = ws + o.f, rb = ws + o.rb + (size_t)l * cs_tld(T);
    const int j0 = blockIdx.x * SUSIE_RR + 2 * wave;
    const int ja = min(j0, rows - 1), jb = min(j0 + 1, rows - 1);
    const auto ra = ja < M ? pb.A + (size_t)ja * ld : pb.B21 + (size_t)(ja - M) * ld;
    const auto rc = jb < M ? pb.A + (size_t)jb * ld : pb.B21 + (size_t)(jb - M) * ld;
    double acc0 = 0.0, acc1 = 0.0;
    for (int i = lane; i < M; i += 64) {
        const double x = v[i];
        acc0 += ra[i] * x;
        acc1 += rc[i] * x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { acc0 += __shfl_xor(acc0, off, 64); acc1 += __shfl_xor(acc1, off, 64); }
    if (lane == 0) {
        if (j0 < rows) { f[j0] = (f[j0] - rb[j0]) + acc0; rb[j0] = acc0; }
        if (j0 + 1 < rows) { f[j0 + 1] = (f[j0 + 1] - rb[j0 + 1]) + acc1; rb[j0 + 1] = acc1; }
    }
}

// ---- sets ----
__global__ __launch_bounds__(CS_SET_T) void susie_set_kernel(const Prob* __restrict__ probs, const int* __restrict__ map)
{
    __shared__ double s_row[CS_LDS_T], s_red[CS_SET_NW];
    const Prob& pb = susie_prob(probs, map, blockIdx.y);
    const int tid = threadIdx.x, l = blockIdx.x;
    const int T = pb.M + pb.U, L = pb.susie_L;
    if (l >= L || (int)blockIdx.z > pb.susie_k) return;
    const SusieWs o = susie_ws_of(pb);
    const SusieTrait tr = susie_trait(pb, o, blockIdx.z);
    const size_t tld = (size_t)cs_tld(T);
    double* const g_row = tr.st + o.lbf + (size_t)l * tld;
    uint8_t* const mem = tr.mem + (size_t)l * tld;
    // the row becomes pips where it stands: where the lbf output or the colocalisation is asked, the Bayes factors themselves are kept
    // (a thread copies the entries that it alone reads first below)
    if (pb.susie_lbf || pb.coloc)
        for (int i = tid; i < T; i += CS_SET_T) tr.st[o.keep + (size_t)l * tld + i] = g_row[i];
    double size, mass, lse;
    cs_set_row(g_row, mem, T, pb.susie_coverage, s_row, s_red, tid, size, mass, lse);
    if (tid == 0) {
        const SusieLayout q = susie_layout(T, L, pb.susie_am != 0);
        tr.out[q.size + l] = size; tr.out[q.mass + l] = mass;
        tr.st[o.lse_set + l] = lse;
    }
}

__global__ __launch_bounds__(SUSIE_T) void susie_rank_kernel(const Prob* __restrict__ probs, const int* __restrict__ map)
{
    const Prob& pb = susie_prob(probs, map, blockIdx.y);
    const int tid = threadIdx.x, l = blockIdx.x;
    const int T = pb.M + pb.U, L = pb.susie_L;
    if (l >= L || (int)blockIdx.z > pb.susie_k) return;
    const SusieWs o = susie_ws_of(pb);
    const SusieTrait tr = susie_trait(pb, o, blockIdx.z);
    const size_t tld = (size_t)cs_tld(T);
    const auto row = tr.st + o.lbf + (size_t)l * tld;      // pips by now (cs_set_row)
    const auto mem = tr.mem + (size_t)l * tld;
    const auto top = (GP(int))(tr.st + o.top) + l * SUSIE_P;
    // the members are a prefix of the order (pip descending, index ascending): a member's place in it is its rank among all candidates
    for (int i = tid; i < T; i += SUSIE_T) {
        if (!mem[i]) continue;
        const double p = row[i];
        int rank = 0;
        for (int j = 0; j < T; j++) {
            const double q = row[j];
            if (q > p || (q == p && j < i)) rank++;
        }
        if (rank < SUSIE_P) top[rank] = i;
    }
    if (tid == 0) {
        const SusieLayout q = susie_layout(T, L, pb.susie_am != 0);
        const double size = tr.out[q.size + l];
        tr.st[o.ntop + l] = size >= 0.0 && size < (double)SUSIE_P ? size : (double)SUSIE_P;
    }
}

__global__ __launch_bounds__(SUSIE_T) void susie_purity_kernel(const Prob* __restrict__ probs, const int* __restrict__ map, int max_L)
{
    __shared__ double s_min[SUSIE_NW];
    __shared__ int s_top[SUSIE_P];
    const Prob& pb = susie_prob(probs, map, blockIdx.z);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.x, l = blockIdx.y % max_L, t = blockIdx.y / max_L;      // (effect, trait) of the job's most effects
    const int M = pb.M, U = pb.U, T = M + U, L = pb.susie_L, ld = pb.Mld;
    if (l >= L || t > pb.susie_k) return;
    const SusieWs o = susie_ws_of(pb);
    const auto ws = pb.susie_ws + (size_t)t * o.trait;      // the trait's state
    const double np = ws[o.ntop + l];
    const int P = __builtin_amdgcn_readfirstlane(np >= 0.0 && np <= (double)SUSIE_P ? (int)np : 0);
    const auto top = (GP(const int))(ws + o.top) + l * SUSIE_P;
    for (int k = tid; k < SUSIE_P; k += SUSIE_T) {
        const int c = k < P ? top[k] : 0;
        s_top[k] = c >= 0 && c < T ? c : 0;                 // (whatever a window that is not fitted has left there: nothing is indexed outside)
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

__global__ __launch_bounds__(SUSIE_T) void susie_kept_kernel(const Prob* __restrict__ probs, const int* __restrict__ map)
{
    __shared__ double s_red[SUSIE_NW];
    __shared__ int s_kept[SUSIE_L];
    const Prob& pb = susie_prob(probs, map, blockIdx.x);
    const int tid = threadIdx.x;
    const int T = pb.M + pb.U, L = pb.susie_L;
    if ((int)blockIdx.z > pb.susie_k) return;
    const SusieWs o = susie_ws_of(pb);
    const SusieLayout q = susie_layout(T, L, pb.susie_am != 0);
    const SusieTrait tr = susie_trait(pb, o, blockIdx.z);
    const auto ws = tr.st;
    const auto out = tr.out;
    const size_t tld = (size_t)cs_tld(T);
    const int sweeps = susie_sweeps_of(pb, ws + o.ctl);
    const auto Vfin = ws + o.V + (size_t)(sweeps & 1) * SUSIE_L;      // what the last sweep's update left
    for (int l = 0; l < L; l++) {
        const double np = ws[o.ntop + l];
        double purity = np >= 2.0 ? __builtin_inf() : (np == 1.0 ? 1.0 : __builtin_nan(""));
        if (np >= 2.0)
            for (int g = 0; g < SUSIE_PG; g++) { const double t = ws[o.part + (size_t)l * SUSIE_PG + g]; purity = t < purity ? t : purity; }
        bool kept = Vfin[l] > 0.0 && purity >= pb.susie_min_abs_corr;
        // no kept set in front of it has the same members
        for (int k = 0; k < l && kept; k++) {
            if (!s_kept[k] || out[q.size + k] != out[q.size + l]) continue;      // (s_kept[k]: written behind a barrier of iteration k)
            double diff = 0.0;
            for (int i = tid; i < T; i += SUSIE_T) diff += tr.mem[(size_t)k * tld + i] != tr.mem[(size_t)l * tld + i] ? 1.0 : 0.0;
            diff = susie_block_sum(diff, s_red, tid);
            if (diff == 0.0) kept = false;
        }
        __syncthreads();
        if (tid == 0) {
            s_kept[l] = kept ? 1 : 0;
            out[q.V + l] = Vfin[l]; out[q.lse + l] = ws[o.lse + l]; out[q.purity + l] = purity; out[q.kept + l] = kept ? 1.0 : 0.0;
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
    }
}

__global__ __launch_bounds__(SUSIE_T) void susie_fold_kernel(const Prob* __restrict__ probs, const int* __restrict__ map)
{
    const Prob& pb = susie_prob(probs, map, blockIdx.y);
    const int T = pb.M + pb.U, L = pb.susie_L;
    const int c = blockIdx.x * SUSIE_T + threadIdx.x;
    if (c >= T || (int)blockIdx.z > pb.susie_k) return;
    const SusieWs o = susie_ws_of(pb);
    const SusieLayout q = susie_layout(T, L, pb.susie_am != 0);
    const SusieTrait tr = susie_trait(pb, o, blockIdx.z);
    const auto ws = tr.st;
    const auto out = tr.out;
    const size_t tld = (size_t)cs_tld(T);
    double keep = 1.0, best = 0.0;
    int set = -1;
    for (int l = 0; l < L; l++) {
        const double a = ws[o.alpha + (size_t)l * tld + c];
        if (out[q.V + l] > 0.0) keep *= 1.0 - a;
        if (out[q.kept + l] != 0.0 && tr.mem[(size_t)l * tld + c] && (set < 0 || a > best)) { set = l; best = a; }
        if (pb.susie_am) { out[q.alpha + (size_t)l * T + c] = a; out[q.mu + (size_t)l * T + c] = ws[o.mu + (size_t)l * tld + c]; }
        if (pb.susie_lbf) tr.out_lbf[(size_t)l * T + c] = ws[o.keep + (size_t)l * tld + c];
    }
    out[q.pip + c] = 1.0 - keep;
    out[q.set + c] = (double)set;
    out[q.set_pip + c] = best;
}

void launch_susie_w(const Prob* d_probs, const int* d_susiemap, int n, int max_nblk, int max_U, hipStream_t s)
{
    if (n <= 0 || max_U <= 0 || max_nblk <= 0) return;
    const dim3 grid(max_nblk, (max_U + NB - 1) / NB, n);
    hipLaunchKernelGGL(susie_w_kernel, grid, dim3(256), 0, s, d_probs, d_susiemap, 0);
    hipLaunchKernelGGL(susie_w_kernel, grid, dim3(256), 0, s, d_probs, d_susiemap, 1);
}

void launch_susie(const Prob* d_probs, const int* d_susiemap, int n, int max_M, int max_T, int max_L, int max_sweeps, int max_k, bool coloc,
                  hipStream_t s)
{
    if (n <= 0 || max_T <= 0) return;
    const unsigned nt = 1 + max_k;                          // fitted traits: a grid dimension of every launch, never a launch
    hipLaunchKernelGGL(susie_prep_kernel, dim3(64, n, nt), dim3(SUSIE_T), 0, s, d_probs, d_susiemap);
    const dim3 gv((max_M + SUSIE_VR - 1) / SUSIE_VR, n, nt), gr((max_T + SUSIE_RR - 1) / SUSIE_RR, n, nt);
    for (int sweep = 0; sweep < max_sweeps; sweep++)
        for (int l = 0; l < max_L; l++) {
            hipLaunchKernelGGL(susie_ser_v_kernel, gv, dim3(SUSIE_T), 0, s, d_probs, d_susiemap, sweep, l);
            hipLaunchKernelGGL(susie_rb_kernel, gr, dim3(SUSIE_T), 0, s, d_probs, d_susiemap, sweep, l);
        }
    hipLaunchKernelGGL(susie_set_kernel, dim3(max_L, n, nt), dim3(CS_SET_T), 0, s, d_probs, d_susiemap);
    hipLaunchKernelGGL(susie_rank_kernel, dim3(max_L, n, nt), dim3(SUSIE_T), 0, s, d_probs, d_susiemap);
    hipLaunchKernelGGL(susie_purity_kernel, dim3(SUSIE_PG, max_L * nt, n), dim3(SUSIE_T), 0, s, d_probs, d_susiemap, max_L);
    hipLaunchKernelGGL(susie_kept_kernel, dim3(n, 1, nt), dim3(SUSIE_T), 0, s, d_probs, d_susiemap);
    if (coloc) launch_coloc(d_probs, d_susiemap, n, max_L, max_k, s);
    hipLaunchKernelGGL(susie_fold_kernel, dim3((max_T + SUSIE_T - 1) / SUSIE_T, n, nt), dim3(SUSIE_T), 0, s, d_probs, d_susiemap);
}

// Single launches of the kernels above over the windows of a map, trait 0 only: the joint fit across studies (k_xsusie.hip) runs the
// state, R bbar_l, the sets' membership and the fold as they are, around a single-effect update of its own.
void launch_susie_prep(const Prob* d_probs, const int* d_map, int n, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(susie_prep_kernel, dim3(64, n, 1), dim3(SUSIE_T), 0, s, d_probs, d_map);
}
void launch_susie_rb(const Prob* d_probs, const int* d_map, int n, int max_T, int sweep, int l, hipStream_t s)
{
    if (n > 0 && max_T > 0)
        hipLaunchKernelGGL(susie_rb_kernel, dim3((max_T + SUSIE_RR - 1) / SUSIE_RR, n, 1), dim3(SUSIE_T), 0, s, d_probs, d_map, sweep, l);
}
void launch_susie_sets(const Prob* d_probs, const int* d_map, int n, int max_L, hipStream_t s)
{
    if (n <= 0 || max_L <= 0) return;
    hipLaunchKernelGGL(susie_set_kernel, dim3(max_L, n, 1), dim3(CS_SET_T), 0, s, d_probs, d_map);
    hipLaunchKernelGGL(susie_rank_kernel, dim3(max_L, n, 1), dim3(SUSIE_T), 0, s, d_probs, d_map);
}
void launch_susie_fold(const Prob* d_probs, const int* d_map, int n, int max_T, hipStream_t s)
{
    if (n > 0 && max_T > 0)
        hipLaunchKernelGGL(susie_fold_kernel, dim3((max_T + SUSIE_T - 1) / SUSIE_T, n, 1), dim3(SUSIE_T), 0, s, d_probs, d_map);
}

}  // namespace gauss
