// kge_interacte.hip -- the body of InteractE (models/projection.py:347-505) in front of the 1-N head of kge_head.hip.
// For a row with entity e and relation r, K = reshape_width * reshape_height, H = 2 reshape_width, W = reshape_height (H W = 2K),
// P = feature_permutation, NF = num_filters, ks = kernel_size, pad = ks / 2, T = ks^2, C = P NF, F = C H W:
//     comb   = [ent[e] | rel[r]]                                 2K values; ONE relation table [R, K]
//     img[p] = comb[perm[p, :]] viewed [H, W]                    p in [0, P): the chequer permutations
//     y0     = bn0(img) * m0                                     a channel per permutation; input dropout, site 0
//     c[p NF + f, y, x] = sum_{i, j < ks} filt[f, i, j] y0[p, (y + i - pad) mod H, (x + j - pad) mod W]
//                                                                depthwise, the SAME NF filters for every p, no bias, circular in both
//                                                                dimensions; VALU from a circularly padded copy of y0[p] in LDS
//                                                                (k_interacte_conv: one workgroup per row and permutation); STORED once
//     A      = relu(bn1(c)) * m1                                 feature-map dropout, site 1: a whole channel of a row; never stored (the
//                                                                [N, C] factors are)
//     u      = A fc_w^T + fc_b                                   [n, F] x [F, K] on v_mfma_f32_16x16x4_f32, F split over workgroups
//                                                                (k_interacte_fc), the partial tiles added in split order (k_interacte_fc_finish)
//     x      = relu(bn2(u * m2))                                 hidden dropout, site 2; bn2 in BOTH forms (eval: running statistics)
// A direction selects nothing.  Training form: every batch norm normalises with the statistics of ITS DIRECTION's n rows and updates
// its running buffers, the tail direction first.  Statistics are fixed-order sums: per-row (mean, M2) partials over equal counts,
// combined over the rows in index order with the equal-count form of Chan's rule, as kge_conve.hip does.  Every row of perm is a
// permutation of [0, 2K) (the host checks it), so the P channels of bn0 see the same 2K values of a row in another order: their
// (mean, M2) partial is formed ONCE per row, over comb in its own order, and serves every p.  Eval form (template parameter TRAIN =
// false): running statistics in bn0, bn1 and bn2, no draws, no writes.
//
// A call works on `dirs` directions of n rows each (body entry points: 1; fused step and rank pass: 2) in the SAME launches: row
// d n + b belongs to direction d.
//
// Backward (training form only), dx the gradient at x:
//     k_interacte_bn2_bwd     du = d loss / d u through relu, bn2 and m2; g_bn2, g_fc_b
//     k_interacte_fc_gw       g_fc[j, f] += sum_b du[b, j] A[b, f]     du^T x A on the matrix cores, ONE owner per output tile walking all rows in order
//     k_interacte_fc_da       dy1 = (du x fc_w) * m1 [bn1 > 0]         du x fc_w on the matrix cores, contraction over K
//     k_interacte_bn1_part / k_interacte_bn1_bwd_fin                   the two sums of bn1's backward, g_bn1
//     k_interacte_conv_gw     per row and permutation: dc from dy1 (in place) and the filter sums gfp[row, p, f, t] = sum_pos dc[pos]
//                             y0[pos shifted by tap t]
//     k_interacte_conv_dx     per row and permutation: the circular correlation of dc with the flipped filters into dy0 (times m0)
//     k_interacte_small_fin   g_conv_filt[f, t] += the (row, p) partials in index order -- the sum over p of the shared filter -- and
//                             bn0's two sums per permutation with g_bn0
//     k_interacte_dcomb       d comb[b, j] = sum_p (bn0's backward of dy0)[b, p, inv_perm[p, j]], p ascending -> dent | drel rows
//     k_interacte_scatter     adds the rows to g_ent[e] / g_rel[r] in row order (no atomics: the wave of the FIRST row that names an
//                             id owns it); every id is scattered, id 0 included (no padding_idx)
// No kernel of this file uses atomics.
//
// The dropout draw is the shared one (kge_projection.h spells the Philox counters out), with
//     site 0: elem = p H W + pixel in [0, 2K P);   site 1: elem = channel in [0, C), one draw per row and channel;   site 2: elem = j in [0, K)
//     row = row0 + position in the call's row list.  The fused step numbers the h rows 0 .. B-1 and the t rows B .. 2B-1.
#include "kge_projection.h"
#include "kge_mfma_blocks.h"

namespace kge {

constexpr int kItMaxK = KGE_INTERACTE_MAX_HIDDEN;    // K: the 2K pixels of a permutation, padded and as four channels of dc, in LDS (k_interacte_conv_gw / k_interacte_conv_dx)
constexpr int kItMaxKs = KGE_INTERACTE_MAX_KERNEL;   // ks: a filter's taps per wave in LDS
constexpr int kItMaxT = 128;                         // >= kItMaxKs^2
constexpr int kItPadMax = 6 * kItMaxK + 256;         // floats of the circularly padded image: (H + 2 pad)(W + 2 pad) with pad <= min(H, W, 5),
                                                     // H W <= 2 kItMaxK is at most 3 H W + 150 (W <= 5) or H W + 10 (H + W) + 100 (both > 5); it_check tests it
constexpr int kItRows = 64;         // batch rows of a matrix-core tile: four 16-row blocks
constexpr int kItKC = 128;          // contraction elements staged in LDS at a time
constexpr int kItStride = 68;       // LDS row stride of the staged tile: 16-byte aligned rows, consecutive rows 4 banks apart
static_assert(kItMaxKs * kItMaxKs <= kItMaxT && kItMaxKs / 2 <= 5, "taps");

struct ItArgs {
    const float *ent, *rel, *w0, *b0, *w1, *b1, *w2, *b2, *fcw, *fcb, *filt;
    const int32_t *perm, *inv;
    int K, H, W, HW, P, NF, ks, pad, T, C, F, Wp, PS;   // Wp = W + 2 pad, PS = (H + 2 pad) Wp
    int dirs;
    int64_t n;                      // rows per direction
    uint32_t row0;
    int on[3];                      // site draws (training form and p > 0)
    DropKey key;
    uint32_t thr[3];
    float scale[3];
    float* stats;                   // [dirs][SS]: mean0[P], rstd0[P], mean1[C], rstd1[C], mean2[K], rstd2[K]
    int SS, o1, o2;                 // SS = 2P + 2C + 2K, o1 = 2P, o2 = 2P + 2C
};
__device__ __forceinline__ const float* it_stats(const ItArgs& a, int d) { return a.stats + (size_t)d * a.SS; }
__device__ __forceinline__ float it_factor(const ItArgs& a, int site, int elem, int64_t gr) {
    return a.on[site] ? drop_row_factor(a.key, site, elem, (int64_t)a.row0 + gr, a.thr[site], a.scale[site]) : 1.0f;
}
__device__ __forceinline__ float it_comb(const ItArgs& a, const float* __restrict__ er, const float* __restrict__ rr, int c) {
    return c < a.K ? er[c] : rr[c - a.K];
}

// one wave per row: (mean, M2) of the row's 2K values [ent[e] | rel[r]]
__global__ void __launch_bounds__(256) k_interacte_row_stats(ItArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                             float2* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t gr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gr >= a.n * a.dirs) return;
    const float* __restrict__ er = a.ent + e[gr] * a.K;
    const float* __restrict__ rr = a.rel + r[gr] * a.K;
    float s = 0.0f;
    for (int c = lane; c < a.HW; c += 64) s += it_comb(a, er, rr, c);
    const float mean = wave_sum_xor(s) / (float)a.HW;
    float m2 = 0.0f;
    for (int c = lane; c < a.HW; c += 64) { const float v = it_comb(a, er, rr, c) - mean; m2 += v * v; }
    m2 = wave_sum_xor(m2);
    if (lane == 0) part[gr] = make_float2(mean, m2);
}

// one wave per channel: the statistics of every direction from the per-row partials part[row * pstride + c * pmul] (each over cnt
// values), the tail direction first; mean / rstd -> stats, running buffers updated (momentum, unbiased variance).  bn0: pstride 1,
// pmul 0 (one partial per row serves every permutation channel); bn1: pstride C, pmul 1
__global__ void __launch_bounds__(256) k_interacte_bn_fin(ItArgs a, const float2* __restrict__ part, int chans, int pstride, int pmul, int cnt,
                                                          int mean_at, int rstd_at, float eps, float mom, float* __restrict__ run_mean,
                                                          float* __restrict__ run_var) {
    const int lane = threadIdx.x & 63;
    const int c = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= chans) return;
    for (int d = 0; d < a.dirs; ++d) {
        const float2* __restrict__ p = part + (size_t)d * a.n * pstride + (size_t)c * pmul;
        float s = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) s += p[b * pstride].x;
        const float mean = wave_sum_xor(s) / (float)a.n;
        float m2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) { const float2 v = p[b * pstride]; const float dv = v.x - mean; m2 += v.y + (float)cnt * (dv * dv); }
        m2 = wave_sum_xor(m2);
        const float tot = (float)a.n * (float)cnt;
        if (lane == 0) {
            float* st = a.stats + (size_t)d * a.SS;
            st[mean_at + c] = mean;
            st[rstd_at + c] = 1.0f / sqrtf(m2 / tot + eps);
            run_mean[c] = (1.0f - mom) * run_mean[c] + mom * mean;
            run_var[c] = (1.0f - mom) * run_var[c] + mom * (m2 / (tot - 1.0f));
        }
    }
}

// eval form: bn0, bn1 and bn2 normalise with the running buffers
__global__ void __launch_bounds__(256) k_interacte_stats_eval(ItArgs a, float eps0, float eps1, float eps2, const float* __restrict__ rm0,
                                                              const float* __restrict__ rv0, const float* __restrict__ rm1,
                                                              const float* __restrict__ rv1, const float* __restrict__ rm2,
                                                              const float* __restrict__ rv2) {
    const int t0 = (int)blockIdx.x * 256 + threadIdx.x;
    for (int d = 0; d < a.dirs; ++d) {
        float* st = a.stats + (size_t)d * a.SS;
        for (int t = t0; t < a.P + a.C + a.K; t += (int)gridDim.x * 256) {
            if (t < a.P) { st[t] = rm0[t]; st[a.P + t] = 1.0f / sqrtf(rv0[t] + eps0); }
            else if (t < a.P + a.C) { const int c = t - a.P; st[a.o1 + c] = rm1[c]; st[a.o1 + a.C + c] = 1.0f / sqrtf(rv1[c] + eps1); }
            else { const int j = t - a.P - a.C; st[a.o2 + j] = rm2[j]; st[a.o2 + a.K + j] = 1.0f / sqrtf(rv2[j] + eps2); }
        }
    }
}

// y0[p] = bn0(comb[perm[p, :]]) * m0 of row gr as a circularly padded [H + 2 pad][W + 2 pad] image in LDS (the wrap-around is a copy
// inside LDS; nothing padded exists in global memory).  All 256 threads; ends with a barrier
__device__ __forceinline__ void it_load_image(const ItArgs& a, const float* __restrict__ st, const int64_t* __restrict__ e,
                                              const int64_t* __restrict__ r, int64_t gr, int p, bool train, float* __restrict__ pimg) {
    const float mean0 = st[p], g0 = st[a.P + p] * a.w0[p], b0 = a.b0[p];
    const float* __restrict__ er = a.ent + e[gr] * a.K;
    const float* __restrict__ rr = a.rel + r[gr] * a.K;
    const int32_t* __restrict__ pp = a.perm + (size_t)p * a.HW;
    for (int pix = threadIdx.x; pix < a.HW; pix += 256) {
        const int y = pix / a.W, x = pix - y * a.W;
        const float val = it_comb(a, er, rr, pp[pix]);
        float v = (val - mean0) * g0 + b0;
        if (train) v *= it_factor(a, 0, p * a.HW + pix, gr);
        pimg[(y + a.pad) * a.Wp + x + a.pad] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < a.PS; idx += 256) {
        const int yp = idx / a.Wp, xp = idx - yp * a.Wp;
        int y = yp - a.pad, x = xp - a.pad;
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) continue;   // (interior: written above, and the only source below)
        if (y < 0) y += a.H; else if (y >= a.H) y -= a.H;        // (pad <= min(H, W): one wrap lands inside)
        if (x < 0) x += a.W; else if (x >= a.W) x -= a.W;
        pimg[idx] = pimg[(y + a.pad) * a.Wp + x + a.pad];
    }
    __syncthreads();
}

// one workgroup per (row, permutation): the padded y0[p] into LDS, then one wave per filter f (its T taps in the wave's LDS slice):
// c[p NF + f, pos] -> conv[row][F], (training form) the channel's (mean, M2) over the row's H W outputs -> part[row][C] and the
// channel's feature-map factor -> m1f[row][C]
template <bool TRAIN>
__global__ void __launch_bounds__(256) k_interacte_conv(ItArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                        float* __restrict__ conv, float2* __restrict__ part, float* __restrict__ m1f) {
    __shared__ float pimg[kItPadMax];
    __shared__ float taps[4][kItMaxT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = (int64_t)blockIdx.x / a.P;
    const int p = (int)((int64_t)blockIdx.x - gr * a.P);
    it_load_image(a, it_stats(a, (int)(gr / a.n)), e, r, gr, p, TRAIN, pimg);
    for (int f0 = 0; f0 < a.NF; f0 += 4) {   // (uniform trip count: the barrier is reached by every wave)
        const int f = f0 + wave;
        __syncthreads();   // (the previous filter's taps have been consumed)
        if (f < a.NF)
            for (int t = lane; t < a.T; t += 64) taps[wave][t] = a.filt[f * a.T + t];
        __syncthreads();
        if (f >= a.NF) continue;
        const int ch = p * a.NF + f;
        float* __restrict__ dst = conv + gr * a.F + (int64_t)ch * a.HW;
        float s = 0.0f;
        for (int pos = lane; pos < a.HW; pos += 64) {
            const int y = pos / a.W, x = pos - y * a.W;
            const float* __restrict__ src = pimg + y * a.Wp + x;
            float v = 0.0f;
            for (int i = 0; i < a.ks; ++i)
                for (int j = 0; j < a.ks; ++j) v += taps[wave][i * a.ks + j] * src[i * a.Wp + j];
            dst[pos] = v;
            s += v;
        }
        if constexpr (TRAIN) {
            const float mean = wave_sum_xor(s) / (float)a.HW;
            float m2 = 0.0f;
            for (int pos = lane; pos < a.HW; pos += 64) { const float v = dst[pos] - mean; m2 += v * v; }   // (written by this lane above)
            m2 = wave_sum_xor(m2);
            if (lane == 0) {
                part[gr * a.C + ch] = make_float2(mean, m2);
                m1f[gr * a.C + ch] = it_factor(a, 1, ch, gr);
            }
        }
    }
}

// y1 = bn1(conv) before the relu, and A[row][f] = relu(y1) * m1, formed from the stored conv output
__device__ __forceinline__ float it_bn1(const ItArgs& a, const float* __restrict__ st, const float* __restrict__ conv, int64_t gr, int f, int ch) {
    return (conv[gr * a.F + f] - st[a.o1 + ch]) * (st[a.o1 + a.C + ch] * a.w1[ch]) + a.b1[ch];
}
template <bool TRAIN>
__device__ __forceinline__ float it_feature(const ItArgs& a, const float* __restrict__ st, const float* __restrict__ conv,
                                            const float* __restrict__ m1f, int64_t gr, int f) {
    const int ch = f / a.HW;
    float v = fmaxf(it_bn1(a, st, conv, gr, f, ch), 0.0f);
    if constexpr (TRAIN) v *= m1f[gr * a.C + ch];
    return v;
}

// upart[split][row][j] = sum over the split's f of A[row][f] fc_w[j][f].  grid (dirs x row tiles, tiles of 64 j, splits of F): wave w
// owns columns 16 (4 blockIdx.y + w) + l; the A tile of 64 rows x 128 f is staged in LDS in the layout read_blocks<4> reads.
template <bool TRAIN>
__global__ void __launch_bounds__(256) k_interacte_fc(ItArgs a, const float* __restrict__ conv, const float* __restrict__ m1f, int tiles, int f_per,
                                                      float* __restrict__ upart) {
    __shared__ float As[kItKC * kItStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int d = (int)blockIdx.x / tiles;
    const int64_t b0 = (int64_t)((int)blockIdx.x % tiles) * kItRows, gr0 = (int64_t)d * a.n + b0;
    const float* __restrict__ st = it_stats(a, d);
    const int j = 16 * ((int)blockIdx.y * 4 + wave) + l, jc = min(j, a.K - 1);
    const int f_lo = (int)blockIdx.z * f_per, f_hi = min(a.F, f_lo + f_per);
    const float* __restrict__ wp = a.fcw + (int64_t)jc * a.F;
    f32x4v acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int fc0 = f_lo; fc0 < f_hi; fc0 += kItKC) {
        const int kn = min(kItKC, f_hi - fc0), kn4 = (kn + 3) & ~3;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kItKC * kItRows; idx += 256) {
            const int kl = idx & (kItKC - 1), rl = idx >> 7;   // consecutive threads: consecutive f of one row
            if (kl >= kn4) continue;
            float v = 0.0f;
            if (b0 + rl < a.n && kl < kn) v = it_feature<TRAIN>(a, st, conv, m1f, gr0 + rl, fc0 + kl);
            As[kl * kItStride + 4 * (rl & 15) + (rl >> 4)] = v;
        }
        __syncthreads();
        for (int s = 0; s < kn4; s += 4) {
            const float b = wp[min(fc0 + s + g, a.F - 1)];   // (rows of As beyond the chunk are zero)
            float av[4];
            read_blocks<4>(&As[(s + g) * kItStride], l, av);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], b, acc[mb], 0, 0, 0);
        }
    }
    if (j >= a.K) return;
    float* __restrict__ dst = upart + (int64_t)blockIdx.z * a.n * a.dirs * a.K;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = b0 + 16 * mb + 4 * g + q;
            if (b < a.n) dst[((int64_t)d * a.n + b) * a.K + j] = acc[mb][q];
        }
}

// one wave per column j: u = fc_b + the partial tiles in split order (kept for the backward); training form: the column's bn2
// statistics per direction over u * m2 (tail first, running buffers updated); x = relu(bn2(u * m2)), in the eval form with the
// running statistics k_interacte_stats_eval left in `stats`
template <bool TRAIN>
__global__ void __launch_bounds__(256) k_interacte_fc_finish(ItArgs a, const float* __restrict__ upart, int splits, float eps, float mom,
                                                             float* __restrict__ run_mean, float* __restrict__ run_var, float* __restrict__ u,
                                                             float* __restrict__ x) {
    const int lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.K) return;
    const int64_t N = a.n * a.dirs;
    const float bias = a.fcb[j];
    for (int d = 0; d < a.dirs; ++d) {
        float* st = a.stats + (size_t)d * a.SS;
        float s = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            float v = bias;
            for (int sp = 0; sp < splits; ++sp) v += upart[((int64_t)sp * N + gr) * a.K + j];
            u[gr * a.K + j] = v;
            if constexpr (TRAIN) s += v * it_factor(a, 2, j, gr);
        }
        float mean, rstd;
        if constexpr (TRAIN) {
            mean = wave_sum_xor(s) / (float)a.n;
            float m2 = 0.0f;
            for (int64_t b = lane; b < a.n; b += 64) {
                const int64_t gr = (int64_t)d * a.n + b;
                const float dv = u[gr * a.K + j] * it_factor(a, 2, j, gr) - mean;   // (u: written by this lane above)
                m2 += dv * dv;
            }
            m2 = wave_sum_xor(m2);
            rstd = 1.0f / sqrtf(m2 / (float)a.n + eps);
            if (lane == 0) {
                st[a.o2 + j] = mean;
                st[a.o2 + a.K + j] = rstd;
                run_mean[j] = (1.0f - mom) * run_mean[j] + mom * mean;
                run_var[j] = (1.0f - mom) * run_var[j] + mom * (m2 / ((float)a.n - 1.0f));
            }
        } else {
            mean = st[a.o2 + j];
            rstd = st[a.o2 + a.K + j];
        }
        const float gj = rstd * a.w2[j], bj = a.b2[j];
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            float v = u[gr * a.K + j];
            if constexpr (TRAIN) v *= it_factor(a, 2, j, gr);
            x[gr * a.K + j] = fmaxf((v - mean) * gj + bj, 0.0f);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// one wave per column j, the directions in order: dy2 = dx [bn2 > 0]; S1 = sum dy2, S2 = sum dy2 xh2; du = w2 rstd (dy2 - S1 / n - xh2 S2 / n) m2
__global__ void __launch_bounds__(256) k_interacte_bn2_bwd(ItArgs a, const float* __restrict__ dx, const float* __restrict__ u, float* __restrict__ du,
                                                           float* __restrict__ g_w2, float* __restrict__ g_b2, float* __restrict__ g_fcb) {
    const int lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.K) return;
    const float w2 = a.w2[j], b2 = a.b2[j];
    for (int d = 0; d < a.dirs; ++d) {
        const float* __restrict__ st = it_stats(a, d);
        const float mean = st[a.o2 + j], rstd = st[a.o2 + a.K + j];
        float s1 = 0.0f, s2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            const float xh = (u[gr * a.K + j] * it_factor(a, 2, j, gr) - mean) * rstd;
            const float dy = xh * w2 + b2 > 0.0f ? dx[gr * a.K + j] : 0.0f;
            s1 += dy;
            s2 += dy * xh;
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        const float inv = 1.0f / (float)a.n;
        float sb = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            const float m = it_factor(a, 2, j, gr);
            const float xh = (u[gr * a.K + j] * m - mean) * rstd;
            const float dy = xh * w2 + b2 > 0.0f ? dx[gr * a.K + j] : 0.0f;
            const float v = (w2 * rstd) * (dy - s1 * inv - xh * (s2 * inv)) * m;
            du[gr * a.K + j] = v;
            sb += v;
        }
        sb = wave_sum_xor(sb);
        if (lane == 0) { g_w2[j] += s2; g_b2[j] += s1; g_fcb[j] += sb; }
    }
}

// g_fc[j][f] += sum over ALL rows (both directions, in row order) of du[row][j] A[row][f].  grid (ceil(F / 64), ceil(K / 128)): wave w
// owns the 16 f of block 4 blockIdx.x + w for the 128 j of blockIdx.y (8 accumulator blocks); the batch is the contraction.  F need
// not be a multiple of 16: a lane beyond F contributes zeros and stores nothing.
__global__ void __launch_bounds__(256) k_interacte_fc_gw(ItArgs a, const float* __restrict__ conv, const float* __restrict__ m1f,
                                                         const float* __restrict__ du, float* __restrict__ g_fc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int f = 16 * ((int)blockIdx.x * 4 + wave) + l;
    if (f - l >= a.F) return;   // (wave-uniform)
    const bool fok = f < a.F;
    const int fcl = min(f, a.F - 1);
    const int k0 = (int)blockIdx.y * 128;
    const int nkb = min(8, (a.K - k0 + 15) / 16);
    const int64_t N = a.n * a.dirs;
    f32x4v acc[8];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) acc[kb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t r0 = 0; r0 < N; r0 += 4) {
        const int64_t gr = r0 + g;
        const bool ok = gr < N;
        const int64_t grc = ok ? gr : N - 1;
        const float v1 = it_feature<true>(a, it_stats(a, (int)(grc / a.n)), conv, m1f, grc, fcl);
        const float A = ok && fok ? v1 : 0.0f;
        const float* __restrict__ dp = du + grc * a.K;
#pragma unroll
        for (int kb = 0; kb < 8; ++kb)
            if (kb < nkb) {
                const int j = k0 + 16 * kb + l;
                const float v = ok && j < a.K ? dp[min(j, a.K - 1)] : 0.0f;
                acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, A, acc[kb], 0, 0, 0);
            }
    }
    if (!fok) return;
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = k0 + 16 * kb + 4 * g + q;
            if (kb < nkb && j < a.K) g_fc[(int64_t)j * a.F + f] += acc[kb][q];
        }
}

// dy1[row][f] = (sum_j du[row][j] fc_w[j][f]) * m1 [bn1 > 0]: the gradient at bn1's output.  grid (dirs x row tiles, ceil(F / 64)):
// wave w owns the 16 f of block 4 blockIdx.y + w for the tile's 64 rows; the du tile (64 rows x 128 j) is staged in LDS as the
// forward's A tile is.
__global__ void __launch_bounds__(256) k_interacte_fc_da(ItArgs a, const float* __restrict__ conv, const float* __restrict__ m1f,
                                                         const float* __restrict__ du, int tiles, float* __restrict__ dy1) {
    __shared__ float As[kItKC * kItStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int d = (int)blockIdx.x / tiles;
    const int64_t b0 = (int64_t)((int)blockIdx.x % tiles) * kItRows, gr0 = (int64_t)d * a.n + b0;
    const float* __restrict__ st = it_stats(a, d);
    const int f = 16 * ((int)blockIdx.y * 4 + wave) + l;
    const bool live = f - l < a.F;   // (wave-uniform)
    const int fcl = min(f, a.F - 1);
    f32x4v acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int j0 = 0; j0 < a.K; j0 += kItKC) {
        const int kn = min(kItKC, a.K - j0), kn4 = (kn + 3) & ~3;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kItKC * kItRows; idx += 256) {
            const int kl = idx & (kItKC - 1), rl = idx >> 7;
            if (kl >= kn4) continue;
            float v = 0.0f;
            if (b0 + rl < a.n && kl < kn) v = du[(gr0 + rl) * a.K + j0 + kl];
            As[kl * kItStride + 4 * (rl & 15) + (rl >> 4)] = v;
        }
        __syncthreads();
        if (live)
            for (int s = 0; s < kn4; s += 4) {
                const float b = a.fcw[(int64_t)min(j0 + s + g, a.K - 1) * a.F + fcl];   // (rows of As beyond the chunk are zero)
                float av[4];
                read_blocks<4>(&As[(s + g) * kItStride], l, av);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], b, acc[mb], 0, 0, 0);
            }
    }
    if (!live || f >= a.F) return;
    const int ch = f / a.HW;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = b0 + 16 * mb + 4 * g + q;
            if (b >= a.n) continue;
            const int64_t gr = (int64_t)d * a.n + b;
            const float keep = it_bn1(a, st, conv, gr, f, ch) > 0.0f ? m1f[gr * a.C + ch] : 0.0f;
            dy1[gr * a.F + f] = acc[mb][q] * keep;
        }
}

// one wave per (row, channel): S1 = sum dy1, S2 = sum dy1 xh1 over the row's H W outputs
__global__ void __launch_bounds__(256) k_interacte_bn1_part(ItArgs a, const float* __restrict__ conv, const float* __restrict__ dy1,
                                                            float2* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    const float* __restrict__ st = it_stats(a, (int)(gr / a.n));
    for (int ch = (int)blockIdx.y * 4 + wave; ch < a.C; ch += 4 * (int)gridDim.y) {
        const float mean = st[a.o1 + ch], rstd = st[a.o1 + a.C + ch];
        const int64_t base = gr * a.F + (int64_t)ch * a.HW;
        float s1 = 0.0f, s2 = 0.0f;
        for (int pos = lane; pos < a.HW; pos += 64) {
            const float dy = dy1[base + pos];
            s1 += dy;
            s2 += dy * ((conv[base + pos] - mean) * rstd);
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        if (lane == 0) part[gr * a.C + ch] = make_float2(s1, s2);
    }
}

// one wave per channel, the directions in order: the two sums over the direction's rows -> sums[d][C], g_bn1
__global__ void __launch_bounds__(256) k_interacte_bn1_bwd_fin(ItArgs a, const float2* __restrict__ part, float2* __restrict__ sums,
                                                               float* __restrict__ g_w1, float* __restrict__ g_b1) {
    const int lane = threadIdx.x & 63;
    const int ch = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ch >= a.C) return;
    for (int d = 0; d < a.dirs; ++d) {
        float s1 = 0.0f, s2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const float2 v = part[((int64_t)d * a.n + b) * a.C + ch];
            s1 += v.x;
            s2 += v.y;
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        if (lane == 0) { sums[d * a.C + ch] = make_float2(s1, s2); g_w1[ch] += s2; g_b1[ch] += s1; }
    }
}

// one workgroup per (row, permutation), one wave per filter f: dc = w1 rstd1 (dy1 - S1 / N1 - xh1 S2 / N1) of channel p NF + f, written
// over dy1 IN PLACE (a lane reads and writes its own positions) and kept in the wave's LDS slice for the filter's T sums
// gfp[row, p, f, t] = sum_pos dc[pos] y0[pos shifted by tap t] (lanes stride the positions, one wave sum per tap)
__global__ void __launch_bounds__(256) k_interacte_conv_gw(ItArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                           const float* __restrict__ conv, float* __restrict__ dy1,
                                                           const float2* __restrict__ sums, float* __restrict__ gfp) {
    __shared__ float pimg[kItPadMax];         // y0[p], circularly padded: what the convolution read
    __shared__ int pbase[2 * kItMaxK];        // pos -> offset of its window's corner in pimg
    __shared__ float dcs[4][2 * kItMaxK];     // dc of the wave's channel
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = (int64_t)blockIdx.x / a.P;
    const int p = (int)((int64_t)blockIdx.x - gr * a.P);
    const int d = (int)(gr / a.n);
    const float* __restrict__ st = it_stats(a, d);
    for (int pos = threadIdx.x; pos < a.HW; pos += 256) { const int y = pos / a.W; pbase[pos] = y * a.Wp + (pos - y * a.W); }
    it_load_image(a, st, e, r, gr, p, true, pimg);
    const float invN1 = 1.0f / ((float)a.n * (float)a.HW);
    for (int f = wave; f < a.NF; f += 4) {   // (no barrier below: a wave works on its own slice of dcs)
        const int ch = p * a.NF + f;
        const float mean = st[a.o1 + ch], rstd = st[a.o1 + a.C + ch], gain = a.w1[ch] * rstd;
        const float2 S = sums[d * a.C + ch];
        const int64_t base = gr * a.F + (int64_t)ch * a.HW;
        for (int pos = lane; pos < a.HW; pos += 64) {
            const float xh = (conv[base + pos] - mean) * rstd;
            const float dc = gain * (dy1[base + pos] - S.x * invN1 - xh * (S.y * invN1));
            dy1[base + pos] = dc;
            dcs[wave][pos] = dc;
        }
        float* __restrict__ gdst = gfp + (((int64_t)gr * a.P + p) * a.NF + f) * a.T;
        for (int i = 0; i < a.ks; ++i)
            for (int j = 0; j < a.ks; ++j) {
                const int off = i * a.Wp + j;
                float s = 0.0f;
                for (int pos = lane; pos < a.HW; pos += 64) s += dcs[wave][pos] * pimg[pbase[pos] + off];   // (dcs: this lane's own writes)
                s = wave_sum_xor(s);
                if (lane == 0) gdst[i * a.ks + j] = s;
            }
    }
}

// one workgroup per (row, permutation).  Four channels at a time (one per wave: dc, left in dy1's place by k_interacte_conv_gw, and
// the filter's taps into LDS); then every thread adds the four channels' circular correlation with the flipped filters to its
// pixels.  dy0 = that sum * m0 -> dimg[row, p][H W]; (sum dy0, sum dy0 xh0) -> pt0[row, p]
__global__ void __launch_bounds__(256) k_interacte_conv_dx(ItArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                           const float* __restrict__ dc, float* __restrict__ dimg, float2* __restrict__ pt0) {
    __shared__ float dcs[4][2 * kItMaxK];     // dc of the four channels in flight
    __shared__ float accs[2 * kItMaxK];       // the correlation's sum per pixel
    __shared__ float fl[4][kItMaxT];
    __shared__ float red[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = (int64_t)blockIdx.x / a.P;
    const int p = (int)((int64_t)blockIdx.x - gr * a.P);
    const float* __restrict__ st = it_stats(a, (int)(gr / a.n));
    for (int c0 = 0; c0 < a.NF; c0 += 4) {
        const int nch = min(4, a.NF - c0);
        __syncthreads();   // (later passes: the previous four channels have been consumed)
        if (wave < nch) {
            const int f = c0 + wave;
            for (int t = lane; t < a.T; t += 64) fl[wave][t] = a.filt[f * a.T + t];
            const int64_t base = gr * a.F + (int64_t)(p * a.NF + f) * a.HW;
            for (int pos = lane; pos < a.HW; pos += 64) dcs[wave][pos] = dc[base + pos];
        }
        __syncthreads();
        for (int pix = threadIdx.x; pix < a.HW; pix += 256) {   // (a thread owns its pixels: accs[pix] is read and written by it alone)
            const int y = pix / a.W, x = pix - y * a.W;
            float v = 0.0f;   // (the four channels' terms first, then ONE addition to the running sum)
            for (int i = 0; i < a.ks; ++i) {
                int yy = y - i + a.pad;
                if (yy < 0) yy += a.H; else if (yy >= a.H) yy -= a.H;   // (pad <= min(H, W): one wrap lands inside)
                for (int j = 0; j < a.ks; ++j) {
                    int xx = x - j + a.pad;
                    if (xx < 0) xx += a.W; else if (xx >= a.W) xx -= a.W;
                    const int idx = yy * a.W + xx, t = i * a.ks + j;
                    for (int w = 0; w < nch; ++w) v += dcs[w][idx] * fl[w][t];
                }
            }
            accs[pix] = c0 ? accs[pix] + v : v;
        }
    }
    const float mean0 = st[p], rstd0 = st[a.P + p];
    const float* __restrict__ er = a.ent + e[gr] * a.K;
    const float* __restrict__ rr = a.rel + r[gr] * a.K;
    const int32_t* __restrict__ pp = a.perm + (size_t)p * a.HW;
    float t1 = 0.0f, t2 = 0.0f;
    for (int pix = threadIdx.x; pix < a.HW; pix += 256) {
        const float v = accs[pix] * it_factor(a, 0, p * a.HW + pix, gr);
        dimg[((int64_t)gr * a.P + p) * a.HW + pix] = v;
        t1 += v;
        t2 += v * ((it_comb(a, er, rr, pp[pix]) - mean0) * rstd0);
    }
    t1 = wave_sum_xor(t1);
    t2 = wave_sum_xor(t2);
    if (lane == 0) { red[wave] = t1; red[4 + wave] = t2; }
    __syncthreads();
    if (threadIdx.x == 0) pt0[gr * a.P + p] = make_float2(((red[0] + red[1]) + red[2]) + red[3], ((red[4] + red[5]) + red[6]) + red[7]);
}

// waves 0 .. NF T - 1: g_conv_filt[f, t] += the (row, p) partials gfp[row, p, f, t] in index order (the filter is shared by the P
// permutations: this is the sum over p); waves NF T .. NF T + P - 1: bn0's two sums per direction -> t0[d][P], g_bn0
__global__ void __launch_bounds__(256) k_interacte_small_fin(ItArgs a, const float* __restrict__ gfp, const float2* __restrict__ pt0,
                                                             float2* __restrict__ t0, float* __restrict__ g_filt, float* __restrict__ g_w0,
                                                             float* __restrict__ g_b0) {
    const int lane = threadIdx.x & 63;
    const int task = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t N = a.n * a.dirs;
    const int Q = a.NF * a.T;
    if (task < Q) {
        const int f = task / a.T, t = task - f * a.T;
        float s = 0.0f;
        for (int64_t q = lane; q < N * a.P; q += 64) s += gfp[(q * a.NF + f) * a.T + t];
        s = wave_sum_xor(s);
        if (lane == 0) g_filt[task] += s;
    } else if (task < Q + a.P) {
        const int p = task - Q;
        for (int d = 0; d < a.dirs; ++d) {
            float s1 = 0.0f, s2 = 0.0f;
            for (int64_t b = lane; b < a.n; b += 64) { const float2 v = pt0[((int64_t)d * a.n + b) * a.P + p]; s1 += v.x; s2 += v.y; }
            s1 = wave_sum_xor(s1);
            s2 = wave_sum_xor(s2);
            if (lane == 0) { t0[d * a.P + p] = make_float2(s1, s2); g_w0[p] += s2; g_b0[p] += s1; }
        }
    }
}

// one workgroup per row: d comb[j] = sum over p, ascending, of bn0's backward of dy0 at the place inv_perm[p, j] where permutation p
// put comb[j]; j < K -> dent[row][j], else drel[row][j - K]
__global__ void __launch_bounds__(256) k_interacte_dcomb(ItArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                         const float* __restrict__ dimg, const float2* __restrict__ t0, float* __restrict__ dent,
                                                         float* __restrict__ drel) {
    const int64_t gr = blockIdx.x;
    const int d = (int)(gr / a.n);
    const float* __restrict__ st = it_stats(a, d);
    const float* __restrict__ er = a.ent + e[gr] * a.K;
    const float* __restrict__ rr = a.rel + r[gr] * a.K;
    const float inv = 1.0f / ((float)a.n * (float)a.HW);
    for (int j = threadIdx.x; j < a.HW; j += 256) {
        const float val = it_comb(a, er, rr, j);
        float acc = 0.0f;
        for (int p = 0; p < a.P; ++p) {
            const float mean0 = st[p], rstd0 = st[a.P + p];
            const float2 T = t0[d * a.P + p];
            const float xh = (val - mean0) * rstd0;
            const float dy = dimg[((int64_t)gr * a.P + p) * a.HW + a.inv[(size_t)p * a.HW + j]];
            acc += (a.w0[p] * rstd0) * (dy - T.x * inv - xh * (T.y * inv));
        }
        if (j < a.K) dent[gr * a.K + j] = acc;
        else drel[gr * a.K + j - a.K] = acc;
    }
}

// dst[ids[b]][0 .. width) += src[b * width .. + width) for every row b (id 0 included: no padding_idx), in row order and without
// atomics: the wave of the FIRST row that names an id owns that id, walks the later rows 64 at a time (ballot) and adds their shares
// in order
__global__ void __launch_bounds__(256) k_interacte_scatter(const int64_t* __restrict__ ids, int64_t n, int width, const float* __restrict__ src,
                                                           float* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int64_t id = ids[row];
    bool dup = false;
    for (int64_t b = lane; b < row; b += 64) dup |= ids[b] == id;
    if (__any(dup)) return;   // (wave-uniform)
    for (int c0 = 0; c0 < width; c0 += 64) {
        const int c = c0 + lane;
        float sum = 0.0f;
        for (int64_t b0 = row & ~(int64_t)63; b0 < n; b0 += 64) {
            const int64_t b = b0 + lane;
            unsigned long long m = __ballot(b >= row && b < n && ids[b] == id);
            while (m) {
                const int64_t s = b0 + __builtin_ctzll(m);
                m &= m - 1;
                if (c < width) sum += src[s * width + c];
            }
        }
        if (c < width) dst[id * width + c] += sum;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
struct ItShape {
    int K, H, W, HW, P, NF, ks, pad, T, C, F, Wp, PS, SS;
};
static ItShape it_shape(const kge_interacte_desc* d) {
    ItShape s{};
    s.K = d->reshape_width * d->reshape_height; s.H = 2 * d->reshape_width; s.W = d->reshape_height; s.HW = 2 * s.K;
    s.P = d->feature_permutation; s.NF = d->num_filters; s.ks = d->kernel_size; s.pad = s.ks / 2; s.T = s.ks * s.ks;
    s.C = s.P * s.NF; s.F = s.C * s.HW; s.Wp = s.W + 2 * s.pad; s.PS = (s.H + 2 * s.pad) * s.Wp; s.SS = 2 * s.P + 2 * s.C + 2 * s.K;
    return s;
}

static int it_check(const kge_interacte_desc* d, const char* who, bool grads) {
    if (!d) { set_error("%s: null descriptor", who); return -1; }
    const void* t[] = {d->bias, d->conv_filt, d->ent, d->rel, d->bn0_w, d->bn0_b, d->bn1_w, d->bn1_b, d->bn2_w, d->bn2_b, d->fc_w, d->fc_b,
                       d->bn0_mean, d->bn0_var, d->bn1_mean, d->bn1_var, d->bn2_mean, d->bn2_var};
    for (const void* p : t)
        if (!p) { set_error("%s: null tables (the 12 parameters and the six running buffers are all required)", who); return -1; }
    if (!d->perm || !d->inv_perm) { set_error("%s: null perm / inv_perm (the chequer permutations and their inverses are required)", who); return -1; }
    if (d->tot_entity <= 0 || d->tot_relation <= 0 || d->reshape_height <= 0 || d->reshape_width <= 0 || d->feature_permutation <= 0 ||
        d->num_filters <= 0 || d->kernel_size <= 0) {
        set_error("%s: tot_entity, tot_relation, reshape_height, reshape_width, feature_permutation, num_filters and kernel_size must be "
                  "positive (got %lld, %lld, %d, %d, %d, %d, %d)", who, (long long)d->tot_entity, (long long)d->tot_relation, d->reshape_height,
                  d->reshape_width, d->feature_permutation, d->num_filters, d->kernel_size);
        return -1;
    }
    if (d->kernel_size < 3 || d->kernel_size % 2 == 0) {
        set_error("%s: kernel_size = %d must be odd and at least 3 (the circular padding of kernel_size / 2 gives an H x W output for odd sizes only)",
                  who, d->kernel_size);
        return -1;
    }
    if (d->kernel_size > kItMaxKs) {
        set_error("%s: kernel_size = %d exceeds %d (a filter's taps are held in LDS)", who, d->kernel_size, kItMaxKs);
        return -1;
    }
    if ((int64_t)d->reshape_height * d->reshape_width > kItMaxK) {
        set_error("%s: reshape_height * reshape_width = %lld exceeds %d (the image and four channels of the conv gradient are held in LDS)", who,
                  (long long)d->reshape_height * d->reshape_width, kItMaxK);
        return -1;
    }
    const int H = 2 * d->reshape_width, W = d->reshape_height, pad = d->kernel_size / 2;
    if (pad > (H < W ? H : W)) {
        set_error("%s: kernel_size / 2 = %d exceeds min(H, W) = %d of the %d x %d image (the circular padding wraps once)", who, pad,
                  H < W ? H : W, H, W);
        return -1;
    }
    if ((H + 2 * pad) * (W + 2 * pad) > kItPadMax) {   // (cannot happen within the limits above; kept as the bound of the LDS image)
        set_error("%s: the padded image of %d floats exceeds %d", who, (H + 2 * pad) * (W + 2 * pad), kItPadMax);
        return -1;
    }
    if ((int64_t)d->feature_permutation * d->num_filters * 2 * d->reshape_height * d->reshape_width > KGE_INTERACTE_MAX_FLAT) {
        set_error("%s: feature_permutation * num_filters * 2 * reshape_height * reshape_width = %lld exceeds %d (feature indices are 32-bit)", who,
                  (long long)d->feature_permutation * d->num_filters * 2 * d->reshape_height * d->reshape_width, KGE_INTERACTE_MAX_FLAT);
        return -1;
    }
    for (int i = 0; i < 3; ++i) {
        if (!(d->momentum[i] > 0.0f && d->momentum[i] <= 1.0f)) {
            set_error("%s: momentum %d must be in (0, 1] (got %g; the cumulative average is not built)", who, i, (double)d->momentum[i]);
            return -1;
        }
        if (!(d->eps[i] >= 0.0f)) { set_error("%s: eps %d must not be negative (got %g)", who, i, (double)d->eps[i]); return -1; }
    }
    const float p[3] = {d->input_dropout, d->feature_map_dropout, d->hidden_dropout};
    if (drop_check(who, p, 3, d->offset)) return -1;
    if (grads) {
        const void* g[] = {d->g_bias, d->g_conv_filt, d->g_ent, d->g_rel, d->g_bn0_w, d->g_bn0_b, d->g_bn1_w, d->g_bn1_b, d->g_bn2_w, d->g_bn2_b,
                           d->g_fc_w, d->g_fc_b};
        for (const void* q : g)
            if (!q) { set_error("%s: null gradient buffers (all 12 are required)", who); return -1; }
    }
    return 0;
}
// rows per direction of a call in training form
static int it_check_rows(const kge_interacte_desc* d, const char* who, int64_t n) {
    if (d->train && n == 1) {
        set_error("%s: batch norm in training form needs more than one row per direction (got n = 1)", who);
        return -1;
    }
    return 0;
}

static ItArgs it_args(const kge_interacte_desc* d, int64_t n, int dirs, int64_t row0, float* stats) {
    const ItShape s = it_shape(d);
    ItArgs a{};
    a.ent = d->ent; a.rel = d->rel; a.w0 = d->bn0_w; a.b0 = d->bn0_b; a.w1 = d->bn1_w; a.b1 = d->bn1_b; a.w2 = d->bn2_w; a.b2 = d->bn2_b;
    a.fcw = d->fc_w; a.fcb = d->fc_b; a.filt = d->conv_filt; a.perm = d->perm; a.inv = d->inv_perm;
    a.K = s.K; a.H = s.H; a.W = s.W; a.HW = s.HW; a.P = s.P; a.NF = s.NF; a.ks = s.ks; a.pad = s.pad; a.T = s.T; a.C = s.C; a.F = s.F;
    a.Wp = s.Wp; a.PS = s.PS; a.SS = s.SS; a.o1 = 2 * s.P; a.o2 = 2 * s.P + 2 * s.C;
    a.dirs = dirs; a.n = n; a.row0 = (uint32_t)row0;
    a.key = drop_key(d->seed, d->offset);
    const float p[3] = {d->input_dropout, d->feature_map_dropout, d->hidden_dropout};
    for (int i = 0; i < 3; ++i) {
        a.on[i] = d->train != 0 && p[i] > 0.0f;
        a.thr[i] = drop_thr(p[i]);
        a.scale[i] = drop_scale(p[i]);
    }
    a.stats = stats;
    return a;
}

static int it_tiles(int64_t n) { return (int)((n + kItRows - 1) / kItRows); }
// f handled by one workgroup of the fc forward: enough workgroups to fill the device, a function of the shapes alone (the split order
// is the summation order); a multiple of 4
static int it_f_per(const ItShape& s, int64_t n, int dirs) {
    const int64_t base = (int64_t)dirs * it_tiles(n) * ((s.K + 63) / 64);
    int64_t splits = (512 + base - 1) / base;
    if (splits > 64) splits = 64;
    if (splits < 1) splits = 1;
    int per = (int)((s.F + splits - 1) / splits);
    per = (per + 3) & ~3;
    return per < 4 ? 4 : per;
}
static int it_splits(const ItShape& s, int per) { return (s.F + per - 1) / per; }

// saved (floats): conv [N, F] | u [N, K] | m1f [N, C] | stats [dirs][2P + 2C + 2K]
static size_t it_saved_floats(const kge_interacte_desc* d, int64_t n, int dirs) {
    const ItShape s = it_shape(d);
    return (size_t)dirs * ((size_t)n * ((size_t)s.F + s.K + s.C) + s.SS);
}
// forward: row partials float2 [N, max(C, 1)] | upart [splits, N, K]
static size_t it_fwd_bytes(const kge_interacte_desc* d, int64_t n, int dirs) {
    const ItShape s = it_shape(d);
    const size_t N = (size_t)n * dirs;
    return align256(N * s.C * sizeof(float2)) + align256((size_t)it_splits(s, it_f_per(s, n, dirs)) * N * s.K * sizeof(float));
}
// backward: du [N, K] | dy1 [N, F] | part1 float2 [N, C] | sums float2 [dirs, C] | gfp [N, P, NF, T] | dimg [N, P, HW] | dent [N, K] | drel [N, K] |
// pt0 float2 [N, P] | t0 float2 [dirs, P]
struct ItBwdPlan {
    size_t du, dy1, part1, sums, gfp, dimg, dent, drel, pt0, t0, total;
};
static ItBwdPlan it_bwd_plan(const kge_interacte_desc* d, int64_t n, int dirs) {
    const ItShape s = it_shape(d);
    const size_t N = (size_t)n * dirs;
    ItBwdPlan p{};
    p.du = 0;
    p.dy1 = p.du + align256(N * s.K * sizeof(float));
    p.part1 = p.dy1 + align256(N * s.F * sizeof(float));
    p.sums = p.part1 + align256(N * s.C * sizeof(float2));
    p.gfp = p.sums + align256((size_t)dirs * s.C * sizeof(float2));
    p.dimg = p.gfp + align256(N * s.P * s.NF * s.T * sizeof(float));
    p.dent = p.dimg + align256(N * s.P * s.HW * sizeof(float));
    p.drel = p.dent + align256(N * s.K * sizeof(float));
    p.pt0 = p.drel + align256(N * s.K * sizeof(float));
    p.t0 = p.pt0 + align256(N * s.P * sizeof(float2));
    p.total = p.t0 + align256((size_t)dirs * s.P * sizeof(float2));
    return p;
}

static int it_forward(const kge_interacte_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int64_t row0, float* x, float* saved,
                      void* ws, hipStream_t st) {
    const ItShape s = it_shape(d);
    const int64_t N = n * dirs;
    float *conv = saved, *u = conv + N * s.F, *m1f = u + N * s.K, *stats = m1f + N * s.C;
    const ItArgs a = it_args(d, n, dirs, row0, stats);
    float2* part = (float2*)ws;
    float* upart = (float*)((char*)ws + align256((size_t)N * s.C * sizeof(float2)));
    const unsigned row_blocks = (unsigned)((N + 3) / 4);
    const bool train = d->train != 0;
    if (train) {
        hipLaunchKernelGGL(k_interacte_row_stats, dim3(row_blocks), dim3(256), 0, st, a, e, r, part);
        hipLaunchKernelGGL(k_interacte_bn_fin, dim3((unsigned)((s.P + 3) / 4)), dim3(256), 0, st, a, part, s.P, 1, 0, s.HW, 0, s.P, d->eps[0],
                           d->momentum[0], d->bn0_mean, d->bn0_var);
        hipLaunchKernelGGL((k_interacte_conv<true>), dim3((unsigned)(N * s.P)), dim3(256), 0, st, a, e, r, conv, part, m1f);
        if (int rc = check_launch("k_interacte_row_stats / k_interacte_bn_fin / k_interacte_conv")) return rc;
        hipLaunchKernelGGL(k_interacte_bn_fin, dim3((unsigned)((s.C + 3) / 4)), dim3(256), 0, st, a, part, s.C, s.C, 1, s.HW, a.o1, a.o1 + s.C,
                           d->eps[1], d->momentum[1], d->bn1_mean, d->bn1_var);
    } else {
        hipLaunchKernelGGL(k_interacte_stats_eval, dim3((unsigned)((s.P + s.C + s.K + 255) / 256)), dim3(256), 0, st, a, d->eps[0], d->eps[1],
                           d->eps[2], d->bn0_mean, d->bn0_var, d->bn1_mean, d->bn1_var, d->bn2_mean, d->bn2_var);
        hipLaunchKernelGGL((k_interacte_conv<false>), dim3((unsigned)(N * s.P)), dim3(256), 0, st, a, e, r, conv, part, m1f);
    }
    const int per = it_f_per(s, n, dirs), splits = it_splits(s, per), tiles = it_tiles(n);
    const dim3 grid((unsigned)(dirs * tiles), (unsigned)((s.K + 63) / 64), (unsigned)splits);
    const unsigned col_blocks = (unsigned)((s.K + 3) / 4);
    if (train) {
        hipLaunchKernelGGL((k_interacte_fc<true>), grid, dim3(256), 0, st, a, conv, m1f, tiles, per, upart);
        hipLaunchKernelGGL((k_interacte_fc_finish<true>), dim3(col_blocks), dim3(256), 0, st, a, upart, splits, d->eps[2], d->momentum[2],
                           d->bn2_mean, d->bn2_var, u, x);
    } else {
        hipLaunchKernelGGL((k_interacte_fc<false>), grid, dim3(256), 0, st, a, conv, m1f, tiles, per, upart);
        hipLaunchKernelGGL((k_interacte_fc_finish<false>), dim3(col_blocks), dim3(256), 0, st, a, upart, splits, d->eps[2], d->momentum[2],
                           d->bn2_mean, d->bn2_var, u, x);
    }
    return check_launch("k_interacte_fc / k_interacte_fc_finish");
}

static int it_backward(const kge_interacte_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int64_t row0, const float* dx,
                       const float* saved, void* ws, hipStream_t st) {
    const ItShape s = it_shape(d);
    const int64_t N = n * dirs;
    const float *conv = saved, *u = conv + N * s.F, *m1f = u + N * s.K;
    const ItArgs a = it_args(d, n, dirs, row0, const_cast<float*>(m1f + N * s.C));
    const ItBwdPlan p = it_bwd_plan(d, n, dirs);
    char* w = (char*)ws;
    float *du = (float*)(w + p.du), *dy1 = (float*)(w + p.dy1), *gfp = (float*)(w + p.gfp), *dimg = (float*)(w + p.dimg);
    float *dent = (float*)(w + p.dent), *drel = (float*)(w + p.drel);
    float2 *part1 = (float2*)(w + p.part1), *sums = (float2*)(w + p.sums), *pt0 = (float2*)(w + p.pt0), *t0 = (float2*)(w + p.t0);
    const unsigned row_blocks = (unsigned)((N + 3) / 4), col_blocks = (unsigned)((s.K + 3) / 4);
    const int tiles = it_tiles(n);
    const int chan_groups = (s.C + 3) / 4 < 16 ? (s.C + 3) / 4 : 16;
    hipLaunchKernelGGL(k_interacte_bn2_bwd, dim3(col_blocks), dim3(256), 0, st, a, dx, u, du, d->g_bn2_w, d->g_bn2_b, d->g_fc_b);
    hipLaunchKernelGGL(k_interacte_fc_gw, dim3((unsigned)((s.F + 63) / 64), (unsigned)((s.K + 127) / 128)), dim3(256), 0, st, a, conv, m1f, du,
                       d->g_fc_w);
    hipLaunchKernelGGL(k_interacte_fc_da, dim3((unsigned)(dirs * tiles), (unsigned)((s.F + 63) / 64)), dim3(256), 0, st, a, conv, m1f, du, tiles,
                       dy1);
    if (int rc = check_launch("k_interacte_bn2_bwd / k_interacte_fc_gw / k_interacte_fc_da")) return rc;
    hipLaunchKernelGGL(k_interacte_bn1_part, dim3((unsigned)N, (unsigned)chan_groups), dim3(256), 0, st, a, conv, dy1, part1);
    hipLaunchKernelGGL(k_interacte_bn1_bwd_fin, dim3((unsigned)((s.C + 3) / 4)), dim3(256), 0, st, a, part1, sums, d->g_bn1_w, d->g_bn1_b);
    hipLaunchKernelGGL(k_interacte_conv_gw, dim3((unsigned)(N * s.P)), dim3(256), 0, st, a, e, r, conv, dy1, sums, gfp);
    hipLaunchKernelGGL(k_interacte_conv_dx, dim3((unsigned)(N * s.P)), dim3(256), 0, st, a, e, r, dy1, dimg, pt0);
    if (int rc = check_launch("k_interacte_bn1_part / k_interacte_bn1_bwd_fin / k_interacte_conv_gw / k_interacte_conv_dx")) return rc;
    hipLaunchKernelGGL(k_interacte_small_fin, dim3((unsigned)((s.NF * s.T + s.P + 3) / 4)), dim3(256), 0, st, a, gfp, pt0, t0, d->g_conv_filt,
                       d->g_bn0_w, d->g_bn0_b);
    hipLaunchKernelGGL(k_interacte_dcomb, dim3((unsigned)N), dim3(256), 0, st, a, e, r, dimg, t0, dent, drel);
    if (int rc = check_launch("k_interacte_small_fin / k_interacte_dcomb")) return rc;
    hipLaunchKernelGGL(k_interacte_scatter, dim3(row_blocks), dim3(256), 0, st, e, N, s.K, dent, d->g_ent);
    hipLaunchKernelGGL(k_interacte_scatter, dim3(row_blocks), dim3(256), 0, st, r, N, s.K, drel, d->g_rel);
    return check_launch("k_interacte_scatter");
}

static int it_check_ids(const char* who, const kge_interacte_desc* d, const int64_t* e, const int64_t* r, int64_t n, hipStream_t s) {
    return check_er_ids(who, d->tot_entity, d->tot_relation, e, r, n, s);
}

// fused step: ids [4B int64] | x [2B, K] | dx [2B, K] | saved | max(forward, backward, head)
struct ItStepPlan {
    size_t ids, x, dx, saved, rest, total;
};
static ItStepPlan it_step_plan(const kge_interacte_desc* d, int64_t B, int64_t n_hr, int64_t n_tr) {
    ItStepPlan p{};
    const size_t xb = align256((size_t)2 * B * it_shape(d).K * sizeof(float));
    p.ids = 0;
    p.x = align256((size_t)4 * B * sizeof(int64_t));
    p.dx = p.x + xb;
    p.saved = p.dx + xb;
    p.rest = p.saved + align256(it_saved_floats(d, B, 2) * sizeof(float));
    size_t rest = it_fwd_bytes(d, B, 2);
    if (it_bwd_plan(d, B, 2).total > rest) rest = it_bwd_plan(d, B, 2).total;
    const size_t h1 = kge_head_1n_bce_workspace_bytes(B, d->tot_entity, n_hr), h2 = kge_head_1n_bce_workspace_bytes(B, d->tot_entity, n_tr);
    if (h1 > rest) rest = h1;
    if (h2 > rest) rest = h2;
    p.total = p.rest + align256(rest);
    return p;
}

// the rank pass's body (kge_projection.hip): the eval form on the rows [h; t] as two directions; ws = saved | the forward's workspace
static int it_eval_body(const void* desc, const int64_t* e, const int64_t* r, int64_t n, float* x, void* ws, size_t, hipStream_t s) {
    kge_interacte_desc ev = *(const kge_interacte_desc*)desc;
    ev.train = 0;
    const size_t saved = align256(it_saved_floats(&ev, n, 2) * sizeof(float));
    return it_forward(&ev, e, r, n, 2, 0, x, (float*)ws, (char*)ws + saved, s);
}
static ProjectionEval it_eval(const kge_interacte_desc* d, int64_t n) {
    const int64_t rows = n > 0 ? n : 1;
    return ProjectionEval{it_shape(d).K, d->tot_entity, d->tot_relation, d->ent,
                          align256(it_saved_floats(d, rows, 2) * sizeof(float)) + it_fwd_bytes(d, rows, 2), it_eval_body, d->bias};
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_interacte_saved_floats(const kge_interacte_desc* d, int64_t n) {
    return it_check(d, "kge_interacte_saved_floats", false) || n < 0 ? 0 : it_saved_floats(d, n > 0 ? n : 1, 1);
}

size_t kge_interacte_body_forward_workspace_bytes(const kge_interacte_desc* d, int64_t n) {
    return it_check(d, "kge_interacte_body_forward_workspace_bytes", false) || n < 0 ? 0 : it_fwd_bytes(d, n > 0 ? n : 1, 1);
}

int kge_interacte_body_forward(const kge_interacte_desc* d, const int64_t* e, const int64_t* r, int64_t n, int64_t row0, float* x, float* saved,
                               void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_interacte_body_forward";
    if (it_check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!e || !r || !x || !saved)) || row0 < 0 || row0 + n > 0xffffffffLL) {
        set_error("%s: bad arguments (row0 + n below 2^32)", who);
        return -1;
    }
    if (it_check_rows(d, who, n)) return -1;
    if (ws_check(who, workspace, workspace_bytes, it_fwd_bytes(d, n > 0 ? n : 1, 1))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = it_check_ids(who, d, e, r, n, s)) return rc;
    return it_forward(d, e, r, n, 1, row0, x, saved, workspace, s);
}

size_t kge_interacte_body_backward_workspace_bytes(const kge_interacte_desc* d, int64_t n) {
    return it_check(d, "kge_interacte_body_backward_workspace_bytes", false) || n < 0 ? 0 : it_bwd_plan(d, n > 0 ? n : 1, 1).total;
}

int kge_interacte_body_backward(const kge_interacte_desc* d, const int64_t* e, const int64_t* r, int64_t n, int64_t row0, const float* dx,
                                const float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_interacte_body_backward";
    if (it_check(d, who, true)) return -1;
    if (n < 0 || (n > 0 && (!e || !r || !dx || !saved)) || row0 < 0 || row0 + n > 0xffffffffLL) {
        set_error("%s: bad arguments (row0 + n below 2^32)", who);
        return -1;
    }
    if (!d->train) { set_error("%s: the eval form (train = 0) has no backward", who); return -1; }
    if (it_check_rows(d, who, n)) return -1;
    if (ws_check(who, workspace, workspace_bytes, it_bwd_plan(d, n > 0 ? n : 1, 1).total)) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = it_check_ids(who, d, e, r, n, s)) return rc;
    return it_backward(d, e, r, n, 1, row0, dx, saved, workspace, s);
}

size_t kge_interacte_train_bce_workspace_bytes(const kge_interacte_desc* d, int64_t batch, int64_t n_hr, int64_t n_tr) {
    if (it_check(d, "kge_interacte_train_bce_workspace_bytes", false) || batch < 0 || n_hr < 0 || n_tr < 0) return 0;
    return it_step_plan(d, batch > 0 ? batch : 1, n_hr, n_tr).total;
}

int kge_interacte_train_bce(const kge_interacte_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t batch, const int64_t* hr_off,
                            const int32_t* hr_ids, int64_t n_hr, const int64_t* tr_off, const int32_t* tr_ids, int64_t n_tr, float label_smoothing,
                            void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    const char* who = "kge_interacte_train_bce";
    if (it_check(d, who, true)) return -1;
    if (batch < 0 || n_hr < 0 || n_tr < 0 || !loss || (batch > 0 && (!h || !r || !t || !hr_off || !tr_off)) || (n_hr > 0 && !hr_ids) ||
        (n_tr > 0 && !tr_ids) || 2 * batch > 0xffffffffLL) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    if (!d->train) { set_error("%s: the step is the training form (train = 0 has no backward)", who); return -1; }
    if (it_check_rows(d, who, batch)) return -1;
    const ItStepPlan p = it_step_plan(d, batch > 0 ? batch : 1, n_hr, n_tr);
    if (ws_check(who, workspace, workspace_bytes, p.total)) return -1;
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t B = batch, n = 2 * B;
    const int k = it_shape(d).K;
    char* ws = (char*)workspace;
    int64_t* e = (int64_t*)(ws + p.ids);
    int64_t* rr = e + n;
    float *x = (float*)(ws + p.x), *dx = (float*)(ws + p.dx), *saved = (float*)(ws + p.saved);
    void* rest = ws + p.rest;
    const size_t rest_bytes = p.total - p.rest;
    const size_t idb = (size_t)B * sizeof(int64_t);
    if (hipMemcpyAsync(e, h, idb, hipMemcpyDeviceToDevice, s) != hipSuccess || hipMemcpyAsync(e + B, t, idb, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(rr, r, idb, hipMemcpyDeviceToDevice, s) != hipSuccess || hipMemcpyAsync(rr + B, r, idb, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("%s: copying the row ids failed: %s", who, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    if (int rc = it_check_ids(who, d, e, rr, n, s)) return rc;
    // tail direction = forward(h, r, "tail") on rows 0 .. B-1, head direction = forward(t, r, "head") on rows B .. 2B-1, in the same launches
    if (int rc = it_forward(d, e, rr, B, 2, 0, x, saved, rest, s)) return rc;
    if (int rc = kge_head_1n_bce(x, B, k, d->ent, d->tot_entity, d->bias, hr_off, hr_ids, n_hr, label_smoothing, rest, rest_bytes, loss, dx, d->g_ent,
                                 d->g_bias, stream)) return rc;
    if (int rc = kge_head_1n_bce(x + B * k, B, k, d->ent, d->tot_entity, d->bias, tr_off, tr_ids, n_tr, label_smoothing, rest, rest_bytes, loss,
                                 dx + B * k, d->g_ent, d->g_bias, stream)) return rc;
    return it_backward(d, e, rr, B, 2, 0, dx, saved, rest, s);
}

size_t kge_interacte_eval_ranks_workspace_bytes(const kge_interacte_desc* d, int64_t n) {
    return it_check(d, "kge_interacte_eval_ranks_workspace_bytes", false) || n < 0 ? 0 : projection_eval_workspace_bytes(it_eval(d, n), n);
}

int kge_interacte_eval_ranks(const kge_interacte_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                             const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks, int32_t* ties,
                             void* stream) {
    const char* who = "kge_interacte_eval_ranks";
    if (it_check(d, who, false)) return -1;
    return projection_eval_ranks(who, it_eval(d, n), d, triples, n, tail_off, tail_ids, head_off, head_ids, workspace, workspace_bytes, ranks,
                                 ties, stream);
}

}  // extern "C"
