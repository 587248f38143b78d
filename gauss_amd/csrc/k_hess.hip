// Local heritability / genetic covariance of an LD block (HESS, rho-HESS, LAVA): all eigenvalues of the block's LD matrix, which
// an LD-only job left in HBM, and the traits' projections on its leading eigenvectors.  The rule, the outputs and the refusals:
// include/gauss_hip.h (gauss_ld_hess_rows).  M SNPs; np = M rounded up to HESS_PW = 32 columns, ldn = M rounded up to HESS_RC = 64
// rows; Gm and V are column-major [np][ldn], every entry outside the M x M corner an exact zero from the first kernel to the last.
//
// hess_mono_kernel: mono[i] = M > 1 and R_ij is NaN for every j != i (a monomorphic SNP, sumchi2's nanrow); one wave per row.
// hess_prep_kernel: Gm = R' (R with the rows, columns and diagonal of the monomorphic SNPs zero and every other non-finite entry
//     zero), V = I on all M SNPs (a zero column of Gm is never rotated, so its column of V stays the unit vector, an eigenvector
//     of R' to the eigenvalue 0); the repaired z [T][ldn] (0 for a monomorphic SNP, a non-finite value and the padding).  A non-finite entry outside the
//     monomorphic rows is counted once per pair i <= j: a count per thread, summed over the wave by cross-lane moves, one integer
//     atomic per wave (the count does not depend on the order).  R is symmetric in its bits: entry (r, c) is read as R[c][r], one
//     coalesced run per column.
// hess_block_round_kernel: block one-sided (Hestenes) Jacobi on Gm = R' V.  The np / 16 column blocks are paired by the round-robin
//     schedule of jacobi_round_kernel (k_misc.hip), one launch per round, one workgroup of 4 waves per pair = 32 columns:
//     1. S = Gp^T Gp (32 x 32) on v_mfma_f64_16x16x4_f64, wave w the 16 x 16 tile (w >> 1, w & 1); the rows come through LDS in
//        chunks of 64 (one 512-byte run per column); a chunk is a chain of 16 MFMAs from zero over its rows in ascending steps of 4,
//        and the chunks' sums are added pairwise in the fixed tree of a binary counter (chunk c joins level 0, two sums of a level
//        make one of the next, what is left is added from the smallest level up).  One chain over all the rows leaves S_pq with a
//        rounding noise that grows with sqrt(M) and passes the 1e-15 guard below at M = 4 096: the solve then never sees a sweep
//        without a rotation (measured: 30 sweeps, GAUSS_ST_HESS_NOCONV); the tree keeps the noise at that of one chunk.
//        The lower triangle is then overwritten by the upper.
//     2. every |S_pq| <= 1e-15 sqrt(S_pp S_qq) (p < q): the pair is left as it is, nothing is written.  Otherwise S is rotated in LDS
//        by cyclic two-sided Jacobi with the vectors accumulated (Q = I at the start): a sweep is 31 rounds of the 16 disjoint
//        pairs of the round-robin order; a pair is rotated iff |S_pq| > 1e-15 sqrt(S_pp S_qq); the rotation is sumchi2_kernel's
//        (tau, t, c, s), rows then columns, and the columns of Q with them.  A fixed number of sweeps, HESS_INNER_MAX = 1 (a sweep
//        without a rotation would end a longer run): what one sweep leaves is left to the next visit.  Measured at M = 1 213: caps of
//        1 / 2 / 4 sweeps take 18 / 17 / 17 outer sweeps and 139 / 158 / 208 ms a call.
//        The columns of Q are then put in the descending order of the diagonal of S, the new columns' squared norms (de Rijk's
//        ordering on max(diagonal, 0); a tie keeps the order, so nothing ranks behind a zero column and the padding columns stay in place): 20 -> 18 outer sweeps at M = 1 213.
//        A column whose squared norm is at or below null2 = (M 2^-52)^2 is numerically null and is treated as a zero column is: never
//        rotated.  R' has a unit or zero diagonal, so its largest eigenvalue is at most M, and a column g = R' v of that size is the
//        rounding of a zero: in a rank-deficient block (more SNPs than samples) such columns have inner products that are noise of
//        relative size 1, no rotation settles them, and without the floor no sweep is ever free of rotations (measured: M = 600 of 300
//        samples, 30 sweeps and GAUSS_ST_HESS_NOCONV with every eigenpair already good to 1e-14).  Its eigenvalue is within M 2^-52
//        of 0, far below any eig_min > 0 of the largest; its column of V stays a unit vector orthogonal to the others.
//        Then one Newton-Schulz step Q <- Q (3 I - Q^T Q) / 2 in LDS (sums over k = 0 .. 31 ascending): V is multiplied by one Q per
//        visit, and without the step the rotations' rounding in Q^T Q - I adds up in V^T V - I visit after visit.
//     3. Gp <- Gp Q and Vp <- Vp Q on the matrix cores, chunk by chunk in place (a chunk is in LDS whole before its first store):
//        wave w the rows 16 w .. 16 w + 15 of the chunk, two 16 x 16 tiles, K = the 32 old columns in ascending steps of 4.  The
//        workgroup then adds 1 to the rotation counter (an integer atomic).
//     A zero column has S_pq = 0 against every column: it is never rotated, Q holds the unit vector for it, and the products leave
//     it and everyone else's share of it exact zeros.  Why 16 and not 32: the diagonalisation of S is the serial part -- 3 barriers a
//     round, 31 rounds a sweep at 32 columns, 63 at 64 with four times the entries -- while a round at M = 1 213 has 38 pairs at 16
//     and 19 at 32 for 256 CUs; 16 keeps more of the chip busy and S, Q and the chunk in 34 KB of LDS.
// hess_lambda_kernel: lam_j = v_j . g_j with its sign, one workgroup per column: thread t adds the products of the rows t, t + 256,
//     ... in ascending order (one product, one add each), then 8 halving steps part[t] += part[t + s], s = 128 .. 1.
// hess_proj_kernel: proj[t][i] = (v_c . z_t) / sqrt(lam_i), c the solver column of the i-th largest eigenvalue; one workgroup per i,
//     wave w the traits w, w + 4, ...: lane l adds the products V[k][c] z_t[k] of the rows k = l, l + 64, ... < ldn in ascending
//     order (one product, one add each), then the 6 halving steps part[l] += part[l + s], s = 32 .. 1 (an exchange between lanes;
//     addition commutes, so every lane holds the halving tree's sum).  A trait is summed on its own: its value does not depend on T.
// Compiled with -ffp-contract=off.  No floating-point atomics, every sum in a fixed order, nothing waits for another workgroup;
// the launch boundary is the only synchronisation.
#include "gauss_internal.h"
#include "k_solve_common.h"
namespace gauss {

constexpr int HESS_PITCH = HESS_RC + 4;        // doubles between two columns of the staged chunk
constexpr int HESS_SP = HESS_PW + 1;           // doubles between two rows of S and of Q
constexpr int HESS_NP2 = HESS_PW / 2;          // pairs of a round of the inner Jacobi
constexpr int HESS_LEVELS = 7;                 // levels of the pairwise sum of the chunks' Gram products: 2^7 > HESS_M_MAX / HESS_RC chunks
static_assert((1 << HESS_LEVELS) > HESS_M_MAX / HESS_RC, "a level for every bit of the chunk count");
static_assert(HESS_T == 256 && HESS_B == 16 && HESS_PW == 32 && HESS_RC == 64, "hess_block_round_kernel: 4 waves, 2 x 2 tiles of 16 x 16, 64 rows a chunk");

__global__ __launch_bounds__(HESS_T) void hess_mono_kernel(const HessArgs a)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * (HESS_T / 64) + (threadIdx.x >> 6), M = a.M;
    if (i >= M) return;                                     // wave-uniform
    const auto row = G(a.R) + (size_t)i * (size_t)M;
    bool some = false;
    for (int j = lane; j < M; j += 64) some = some || (j != i && !isnan(row[j]));
    const bool any = __ballot(some) != 0ull;
    if (lane == 0) G(a.mono)[i] = (M > 1 && !any) ? 1 : 0;
}

__global__ __launch_bounds__(HESS_T) void hess_prep_kernel(const HessArgs a)
{
    const int M = a.M, ldn = a.ldn;
    const size_t idx = (size_t)blockIdx.x * HESS_T + threadIdx.x;
    const size_t total = (size_t)a.np * (size_t)ldn;
    unsigned cnt = 0;
    if (idx < total) {
        const int r = (int)(idx % (size_t)ldn), c = (int)(idx / (size_t)ldn);
        double g = 0.0;
        if (r < M && c < M && !G(a.mono)[r] && !G(a.mono)[c]) {
            const double x = G(a.R)[(size_t)c * (size_t)M + (size_t)r];
            if (isfinite(x)) g = x;
            else if (r <= c) cnt = 1;
        }
        G(a.Gm)[idx] = g;
        G(a.V)[idx] = (r == c && r < M) ? 1.0 : 0.0;
    }
    // the repaired z (T * ldn entries may be more than the grid has threads: a loop)
    for (size_t e = idx; e < (size_t)a.T * (size_t)ldn; e += (size_t)gridDim.x * HESS_T) {
        const int t = (int)(e / (size_t)ldn), k = (int)(e % (size_t)ldn);
        double v = 0.0;
        if (k < M && !G(a.mono)[k]) {
            const double x = G(a.z)[(size_t)t * (size_t)M + (size_t)k];
            if (isfinite(x)) v = x;
        }
        G(a.zr)[e] = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(a.n_nonfinite, (unsigned long long)cnt);
}

__global__ __launch_bounds__(HESS_T) void hess_block_round_kernel(const HessArgs a, const int round)
{
    __shared__ __attribute__((aligned(16))) double s_t[HESS_PW * HESS_PITCH];      // the chunk: [column of the pair][row of the chunk]
    __shared__ double s_S[HESS_PW * HESS_SP];
    __shared__ double s_Q[HESS_PW * HESS_SP];
    __shared__ double s_c[HESS_NP2], s_s[HESS_NP2];
    __shared__ int s_p[HESS_NP2], s_q[HESS_NP2];
    __shared__ int s_rank[HESS_PW];
    __shared__ int s_flag[2];                               // [0] the pair needs a rotation, [1] the inner sweep made one
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ldn = a.ldn;
    const int m = a.np / HESS_B - 1;                        // the round-robin order over the np / 16 blocks (an even number of them)
    int P, Q;
    if (blockIdx.x == 0) { P = m; Q = round % m; }
    else { P = (round + (int)blockIdx.x) % m; Q = (round - (int)blockIdx.x + m) % m; }
    if (P > Q) { const int x = P; P = Q; Q = x; }
    // thread tid stages the entries e = tid + 256 u of a chunk: column e >> 6 of the pair, row e & 63
    const int st_r = tid & 63;
    size_t st_col[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int c = (tid >> 6) + 4 * u;
        st_col[u] = (size_t)(c < HESS_B ? P * HESS_B + c : Q * HESS_B + c - HESS_B) * (size_t)ldn;
    }
    if (tid < 2) s_flag[tid] = 0;

    // ---- 1. S = Gp^T Gp
    {
        const auto Gm = G(a.Gm);
        const int ti = wave >> 1, tj = wave & 1;
        f64x4 lvl[HESS_LEVELS];                             // lvl[l]: the sum of 2^l whole chunks, or not in use (bit l of the count is 0)
        int n_chunk = 0;
        const double* ap = s_t + (16 * ti + (lane & 15)) * HESS_PITCH + (lane >> 4);
        const double* bp = s_t + (16 * tj + (lane & 15)) * HESS_PITCH + (lane >> 4);
        double nx[8];                                       // the next chunk, on its way while this one is multiplied
#pragma unroll
        for (int u = 0; u < 8; u++) nx[u] = Gm[st_col[u] + (size_t)st_r];
        for (int r0 = 0; r0 < ldn; r0 += HESS_RC) {
#pragma unroll
            for (int u = 0; u < 8; u++) s_t[((tid >> 6) + 4 * u) * HESS_PITCH + st_r] = nx[u];
            __syncthreads();
            if (r0 + HESS_RC < ldn) {
#pragma unroll
                for (int u = 0; u < 8; u++) nx[u] = Gm[st_col[u] + (size_t)(r0 + HESS_RC + st_r)];
            }
            f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k0 = 0; k0 < HESS_RC; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[k0], bp[k0], acc, 0, 0, 0);
            // the chunks' sums meet pairwise, as a binary counter carries: chunk c joins level 0; two sums of a level make one of the next
            bool placed = false;
#pragma unroll
            for (int l = 0; l < HESS_LEVELS; l++) {
                if (placed) continue;
                if ((n_chunk >> l) & 1) acc = lvl[l] + acc;
                else { lvl[l] = acc; placed = true; }
            }
            n_chunk++;
            __syncthreads();
        }
        f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};               // what the levels hold, the smallest (the last chunks) first
        bool first = true;
#pragma unroll
        for (int l = 0; l < HESS_LEVELS; l++) {
            if (!((n_chunk >> l) & 1)) continue;
            acc = first ? lvl[l] : lvl[l] + acc;
            first = false;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) s_S[(16 * ti + (lane >> 4) + 4 * r) * HESS_SP + 16 * tj + (lane & 15)] = acc[r];
    }
    __syncthreads();
    // ---- 2. the guard; the lower triangle from the upper
    {
        bool need = false;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = tid + HESS_T * u, p = e >> 5, q = e & 31;
            if (p < q) {
                const double g = s_S[p * HESS_SP + q];
                const double dp = s_S[p * HESS_SP + p], dq = s_S[q * HESS_SP + q];
                need = need || (fabs(g) > 1e-15 * sqrt(dp * dq) && g != 0.0 && dp > a.null2 && dq > a.null2);
            }
        }
        if (need) s_flag[0] = 1;
    }
    __syncthreads();
    if (!s_flag[0]) return;                                 // uniform: already orthogonal, nothing is written
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int e = tid + HESS_T * u, p = e >> 5, q = e & 31;
        if (p > q) s_S[p * HESS_SP + q] = s_S[q * HESS_SP + p];
        s_Q[p * HESS_SP + q] = p == q ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int sweep = 0; sweep < HESS_INNER_MAX; sweep++) {
        for (int rd = 0; rd < HESS_PW - 1; rd++) {
            if (tid < HESS_NP2) {
                int p, q;
                if (tid == 0) { p = HESS_PW - 1; q = rd; }
                else { p = (rd + tid) % (HESS_PW - 1); q = (rd - tid + HESS_PW - 1) % (HESS_PW - 1); }
                if (p > q) { const int x = p; p = q; q = x; }
                double c = 1.0, s = 0.0;
                const double apq = s_S[p * HESS_SP + q], app = s_S[p * HESS_SP + p], aqq = s_S[q * HESS_SP + q];
                if (fabs(apq) > 1e-15 * sqrt(app * aqq) && apq != 0.0 && app > a.null2 && aqq > a.null2) {
                    const double tau = (aqq - app) / (2.0 * apq);
                    const double tt = fabs(tau) > 1e150 ? 0.5 / tau : (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + tt * tt);
                    s = tt * c;
                    s_flag[1] = 1;
                }
                s_p[tid] = p; s_q[tid] = q; s_c[tid] = c; s_s[tid] = s;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; u++) {                   // rows p, q <- J^T S
                const int e = tid + HESS_T * u, r = e >> 5, j = e & 31;
                const double c = s_c[r], s = s_s[r];
                if (s == 0.0) continue;
                double* rp = s_S + s_p[r] * HESS_SP;
                double* rq = s_S + s_q[r] * HESS_SP;
                const double x = rp[j], y = rq[j];
                rp[j] = c * x - s * y;
                rq[j] = s * x + c * y;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; u++) {                   // columns p, q <- S J, Q J
                const int e = tid + HESS_T * u, r = e >> 5, i = e & 31;
                const double c = s_c[r], s = s_s[r];
                if (s == 0.0) continue;
                const int p = s_p[r], q = s_q[r];
                const double x = s_S[i * HESS_SP + p], y = s_S[i * HESS_SP + q];
                s_S[i * HESS_SP + p] = c * x - s * y;
                s_S[i * HESS_SP + q] = s * x + c * y;
                const double v = s_Q[i * HESS_SP + p], w = s_Q[i * HESS_SP + q];
                s_Q[i * HESS_SP + p] = c * v - s * w;
                s_Q[i * HESS_SP + q] = s * v + c * w;
            }
            __syncthreads();
        }
        const int any = s_flag[1];
        __syncthreads();
        if (!any) break;                                    // uniform
        if (tid == 0) s_flag[1] = 0;                        // (read again only after the next round's first barrier)
    }

    // ---- the columns of Q in the descending order of max(diagonal of S, 0), the squared norms of the new columns; a tie keeps the
    // columns' order.  Nothing ranks behind an exact-zero column, and the zero columns keep their order among themselves: the padding
    // columns, which have the highest indices of all, stay where they are (a monomorphic SNP's column may move towards them)
    {
        double w[4];
        if (tid < HESS_PW) {
            const double d = fmax(s_S[tid * HESS_SP + tid], 0.0);      // (a near-null column's rotated diagonal may round below 0)
            int rank = 0;
            for (int j = 0; j < HESS_PW; j++) {
                const double dj = fmax(s_S[j * HESS_SP + j], 0.0);
                rank += (dj > d || (dj == d && j < tid)) ? 1 : 0;
            }
            s_rank[tid] = rank;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = tid + HESS_T * u;
            w[u] = s_Q[(e >> 5) * HESS_SP + (e & 31)];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = tid + HESS_T * u;
            s_Q[(e >> 5) * HESS_SP + s_rank[e & 31]] = w[u];
        }
        __syncthreads();
    }

    // ---- Q <- Q (3 I - Q^T Q) / 2: one Newton-Schulz step.  The product of some hundred rounded rotations is orthogonal to some tens
    // of ulps only, and V is multiplied by one such Q at every visit; the step leaves Q^T Q = I to the rounding of the step itself.
    // S is no longer needed: its place holds (3 I - Q^T Q) / 2.  Every sum over k = 0 .. 31 in ascending order.
    {
        double w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = tid + HESS_T * u, p = e >> 5, q = e & 31;
            double d = 0.0;
#pragma unroll 8
            for (int k = 0; k < HESS_PW; k++) d = d + s_Q[k * HESS_SP + p] * s_Q[k * HESS_SP + q];
            s_S[p * HESS_SP + q] = (p == q ? 1.5 : 0.0) - 0.5 * d;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = tid + HESS_T * u, i = e >> 5, j = e & 31;
            double d = 0.0;
#pragma unroll 8
            for (int k = 0; k < HESS_PW; k++) d = d + s_Q[i * HESS_SP + k] * s_S[k * HESS_SP + j];
            w[u] = d;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = tid + HESS_T * u;
            s_Q[(e >> 5) * HESS_SP + (e & 31)] = w[u];
        }
        __syncthreads();
    }

    // ---- 3. Gp <- Gp Q, Vp <- Vp Q
    for (int mat = 0; mat < 2; mat++) {
        const auto X = G(mat == 0 ? a.Gm : a.V);
        const double* ap = s_t + (lane >> 4) * HESS_PITCH + 16 * wave + (lane & 15);
        const double* qp = s_Q + (lane >> 4) * HESS_SP + (lane & 15);
        double nx[8];                                       // the next chunk's rows: other rows than the ones being stored
#pragma unroll
        for (int u = 0; u < 8; u++) nx[u] = X[st_col[u] + (size_t)st_r];
        for (int r0 = 0; r0 < ldn; r0 += HESS_RC) {
#pragma unroll
            for (int u = 0; u < 8; u++) s_t[((tid >> 6) + 4 * u) * HESS_PITCH + st_r] = nx[u];
            __syncthreads();
            if (r0 + HESS_RC < ldn) {
#pragma unroll
                for (int u = 0; u < 8; u++) nx[u] = X[st_col[u] + (size_t)(r0 + HESS_RC + st_r)];
            }
            f64x4 acc[2] = {f64x4{0.0, 0.0, 0.0, 0.0}, f64x4{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
            for (int k0 = 0; k0 < HESS_PW; k0 += 4) {
                const double x = ap[k0 * HESS_PITCH];
#pragma unroll
                for (int n = 0; n < 2; n++) acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, qp[k0 * HESS_SP + 16 * n], acc[n], 0, 0, 0);
            }
            __syncthreads();
#pragma unroll
            for (int n = 0; n < 2; n++)
#pragma unroll
                for (int r = 0; r < 4; r++) s_t[(16 * n + (lane & 15)) * HESS_PITCH + 16 * wave + (lane >> 4) + 4 * r] = acc[n][r];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 8; u++) X[st_col[u] + (size_t)(r0 + st_r)] = s_t[((tid >> 6) + 4 * u) * HESS_PITCH + st_r];
            __syncthreads();
        }
    }
    if (tid == 0) atomicAdd(a.n_rot, 1u);
}

__global__ __launch_bounds__(HESS_T) void hess_lambda_kernel(const HessArgs a)
{
    __shared__ double red[HESS_T];
    const int j = blockIdx.x, tid = threadIdx.x;
    const auto g = G(a.Gm) + (size_t)j * (size_t)a.ldn;
    const auto v = G(a.V) + (size_t)j * (size_t)a.ldn;
    double s = 0.0;
    for (int k = tid; k < a.ldn; k += HESS_T) {
        const double pr = v[k] * g[k];
        s = s + pr;
    }
    red[tid] = s;
    __syncthreads();
    for (int h = HESS_T / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    if (tid == 0) G(a.lam)[j] = red[0];
}

__global__ __launch_bounds__(HESS_T) void hess_proj_kernel(const HessArgs a)
{
    const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ldn = a.ldn;
    const auto v = G(a.V) + (size_t)G(a.order)[i] * (size_t)ldn;
    const double root = sqrt(G(a.lam_sorted)[i]);
    for (int t = wave; t < a.T; t += HESS_T / 64) {
        const auto z = G(a.zr) + (size_t)t * (size_t)ldn;
        double s = 0.0;
        for (int k = lane; k < ldn; k += 64) {
            const double pr = v[k] * z[k];
            s = s + pr;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64);
        if (lane == 0) G(a.proj)[(size_t)t * (size_t)a.k_max + i] = s / root;
    }
}

void launch_hess_prep(const HessArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(hess_mono_kernel, dim3((a.M + HESS_T / 64 - 1) / (HESS_T / 64)), dim3(HESS_T), 0, s, a);
    const size_t total = (size_t)a.np * (size_t)a.ldn;
    hipLaunchKernelGGL(hess_prep_kernel, dim3((unsigned)((total + HESS_T - 1) / HESS_T)), dim3(HESS_T), 0, s, a);
}

hipError_t hess_solve(const HessArgs& a, hipStream_t s, int* sweeps, bool* converged)
{
    const int nb = a.np / HESS_B;
    *sweeps = 0;
    *converged = false;
    for (int sweep = 0; sweep < HESS_MAX_SWEEPS; sweep++) {
        hipError_t e = hipMemsetAsync(a.n_rot, 0, sizeof(unsigned int), s);
        if (e != hipSuccess) return e;
        for (int r = 0; r < nb - 1; r++) hipLaunchKernelGGL(hess_block_round_kernel, dim3(nb / 2), dim3(HESS_T), 0, s, a, r);
        e = hipGetLastError();                              // a launch of this sweep that failed ends the solve here
        if (e != hipSuccess) return e;
        unsigned int h_rot = 0;
        e = hipMemcpyAsync(&h_rot, a.n_rot, sizeof(unsigned int), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return e;
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        *sweeps = sweep + 1;
        if (h_rot == 0) { *converged = true; break; }
    }
    return hipGetLastError();
}

void launch_hess_lambda(const HessArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(hess_lambda_kernel, dim3(a.M), dim3(HESS_T), 0, s, a);
}

void launch_hess_proj(const HessArgs& a, hipStream_t s)
{
    if (a.kk <= 0) return;
    hipLaunchKernelGGL(hess_proj_kernel, dim3(a.kk), dim3(HESS_T), 0, s, a);
}

}  // namespace gauss
