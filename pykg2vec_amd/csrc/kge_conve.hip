// kge_conve.hip -- the body of ConvE (models/projection.py:12-125) in front of the 1-N head of kge_head.hip.
// For a row with entity e and relation r on side s (0 = "tail" direction, 1 = "head": relation row r + tot_relation), k = hidden_size,
// h1 = hidden_size_1, h2 = k / h1, image H x W = 2 h2 x h1, conv output OH x OW = (H - 2) x (W - 2), F = 32 OH OW:
//     img  = [ent[e] ; rel[r']]                                   2k pixels, row-major, the entity half first
//     y0   = bn0(img) * m0                                        one channel; input dropout, site 0
//     c    = conv3x3(y0) + conv_b                                 32 channels, VALU from the image in LDS (k_conve_conv); STORED once
//     A    = relu(bn1(c)) * m1                                    feature-map dropout, site 1: a whole channel of a row; never stored
//     u    = A fc_w^T + fc_b                                      [n, F] x [F, k] on v_mfma_f32_16x16x4_f32, F split over workgroups
//                                                                 (k_conve_fc), the partial tiles added in split order (k_conve_fc_finish)
//     x    = relu(bn2(u * m2))                                    hidden dropout, site 2; eval form: x = relu(u), no bn2
// Training form: every batch norm normalises with the statistics of ITS DIRECTION's n rows and updates its running buffers, the
// tail direction first.  Statistics are fixed-order sums: per-row (count, mean, M2) partials (deviations about the row's own mean),
// combined over the rows in index order with the equal-count form of Chan's rule (mean of the means; M2 = sum M2_b + cnt sum
// (mean_b - mean)^2).  Eval form (template parameter TRAIN = false): running statistics, no bn2, no draws.
//
// A call works on `dirs` directions of n rows each (body entry points: 1; fused step and rank pass: 2, sides 0 and 1) in the SAME
// launches: the direction is a range of the row axis, row d n + b belongs to direction d.
//
// Backward (training form only), dx the gradient at x:
//     k_conve_bn2_bwd     du = d loss / d u through relu, bn2 and m2; g_bn2, g_fc_b
//     k_conve_fc_gw       g_fc[j, f] += sum_b du[b, j] A[b, f]     du^T x A on the matrix cores, ONE owner per output tile walking all rows in order
//     k_conve_fc_da       dy1 = (du x fc_w) * m1 * [bn1 > 0]       du x fc_w on the matrix cores, contraction over k
//     k_conve_bn1_part / k_conve_bn1_bwd_fin                       the two sums of bn1's backward, g_bn1
//     k_conve_conv_bwd    per row: dc from dy1, its 9 + 1 filter / bias sums, the transposed convolution into dy0 (VALU, LDS)
//     k_conve_small_fin   g_conv_w, g_conv_b, g_bn0 and bn0's two sums, over the rows in index order
//     k_conve_dimg        through bn0 to the image; k_conve_scatter adds the halves to g_ent[e] / g_rel[r'] in row order (no atomics:
//                         the wave of the FIRST row that names an id owns it, as k_tucker_scatter does)
// No kernel of this file uses atomics: with the head's ordered split-K sums the 13 gradients and the six running buffers of a step
// are bit-identical run to run.  (The loss is the head's: bit-identical at small batches, but from about B = 150 on several of the
// head's workgroups share one striped loss accumulator through float atomics and its last bits can differ.)
//
// The dropout draw is the shared one (kge_projection.h spells the Philox counters out), with
//     site 0: elem = pixel in [0, 2k);   site 1: elem = channel in [0, 32), one draw per row and channel;   site 2: elem = j in [0, k)
//     row = row0 + position in the call's row list.  The fused step numbers the h rows 0 .. B-1 and the t rows B .. 2B-1.
#include "kge_projection.h"
#include "kge_mfma_blocks.h"

namespace kge {

constexpr int kCvMaxK = KGE_CONVE_MAX_HIDDEN;       // hidden_size limit: the image (2k floats) and four channels of dc (< 8k floats) fit 48 KB of LDS
constexpr int kCvCh = 32;           // conv2d_1's output channels
constexpr int kCvRows = 64;         // batch rows of a matrix-core tile: four 16-row blocks
constexpr int kCvKC = 128;          // contraction elements staged in LDS at a time
constexpr int kCvStride = 68;       // LDS row stride of the staged tile: 16-byte aligned rows, consecutive rows 4 banks apart

struct CvArgs {
    const float *ent, *rel, *w0, *b0, *cw, *cb, *w1, *b1, *fcw, *fcb, *w2, *b2;
    int k, W, P, OW, F;             // P = OH * OW
    int dirs, side0;
    int64_t n, R;                   // rows per direction, tot_relation
    uint32_t row0;
    int on[3];                      // site draws (training form and p > 0)
    DropKey key;
    uint32_t thr[3];
    float scale[3];
    float* stats;                   // [dirs][66 + 2k]: mean0, rstd0, mean1[32], rstd1[32], mean2[k], rstd2[k]
};
__device__ __forceinline__ int cv_stat_floats(int k) { return 66 + 2 * k; }
__device__ __forceinline__ const float* cv_stats(const CvArgs& a, int d) { return a.stats + (size_t)d * (66 + 2 * a.k); }
__device__ __forceinline__ float cv_factor(const CvArgs& a, int site, int elem, int64_t gr) {
    return a.on[site] ? drop_row_factor(a.key, site, elem, (int64_t)a.row0 + gr, a.thr[site], a.scale[site]) : 1.0f;
}
// pixel p of row gr (direction d)
__device__ __forceinline__ float cv_pixel(const CvArgs& a, const int64_t* __restrict__ e, const int64_t* __restrict__ r, int64_t gr, int d, int p) {
    return p < a.k ? a.ent[e[gr] * a.k + p] : a.rel[(r[gr] + (int64_t)(a.side0 + d) * a.R) * a.k + p - a.k];
}

// one wave per row: (mean, M2) of the row's 2k pixels
__global__ void __launch_bounds__(256) k_conve_img_stats(CvArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r, float2* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t gr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gr >= a.n * a.dirs) return;
    const int d = (int)(gr / a.n), np = 2 * a.k;
    float s = 0.0f;
    for (int p = lane; p < np; p += 64) s += cv_pixel(a, e, r, gr, d, p);
    const float mean = wave_sum_xor(s) / (float)np;
    float m2 = 0.0f;
    for (int p = lane; p < np; p += 64) { const float v = cv_pixel(a, e, r, gr, d, p) - mean; m2 += v * v; }
    m2 = wave_sum_xor(m2);
    if (lane == 0) part[gr] = make_float2(mean, m2);
}

// one wave per channel: the statistics of every direction from the per-row partials part[row][chans] (each over cnt values), the tail
// direction first; mean / rstd -> stats, running buffers updated (momentum, unbiased variance)
__global__ void __launch_bounds__(256) k_conve_bn_fin(CvArgs a, const float2* __restrict__ part, int chans, int cnt, int mean_at, int rstd_at,
                                                      float eps, float mom, float* __restrict__ run_mean, float* __restrict__ run_var) {
    const int lane = threadIdx.x & 63;
    const int c = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= chans) return;
    for (int d = 0; d < a.dirs; ++d) {
        const float2* __restrict__ p = part + (size_t)d * a.n * chans + c;
        float s = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) s += p[b * chans].x;
        const float mean = wave_sum_xor(s) / (float)a.n;
        float m2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) { const float2 v = p[b * chans]; const float dv = v.x - mean; m2 += v.y + (float)cnt * (dv * dv); }
        m2 = wave_sum_xor(m2);
        const float tot = (float)a.n * (float)cnt;
        if (lane == 0) {
            float* st = a.stats + (size_t)d * (66 + 2 * a.k);
            st[mean_at + c] = mean;
            st[rstd_at + c] = 1.0f / sqrtf(m2 / tot + eps);
            run_mean[c] = (1.0f - mom) * run_mean[c] + mom * mean;
            run_var[c] = (1.0f - mom) * run_var[c] + mom * (m2 / (tot - 1.0f));
        }
    }
}

// eval form: bn0 and bn1 normalise with the running buffers
__global__ void k_conve_stats_eval(CvArgs a, float eps0, float eps1, const float* __restrict__ rm0, const float* __restrict__ rv0,
                                   const float* __restrict__ rm1, const float* __restrict__ rv1) {
    const int t = threadIdx.x;
    if (t > kCvCh) return;
    for (int d = 0; d < a.dirs; ++d) {
        float* st = a.stats + (size_t)d * (66 + 2 * a.k);
        if (t == kCvCh) { st[0] = rm0[0]; st[1] = 1.0f / sqrtf(rv0[0] + eps0); }
        else { st[2 + t] = rm1[t]; st[34 + t] = 1.0f / sqrtf(rv1[t] + eps1); }
    }
}

// one workgroup per row: y0 = bn0(img) * m0 into LDS, then one wave per channel: c = conv3x3(y0) + conv_b -> conv[row][F], and
// (training form) the channel's (mean, M2) over the row's OH * OW outputs -> part[row][32]
template <bool TRAIN>
__global__ void __launch_bounds__(256) k_conve_conv(CvArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r, float* __restrict__ conv,
                                                    float2* __restrict__ part) {
    __shared__ float img[2 * kCvMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    const int d = (int)(gr / a.n);
    const float* __restrict__ st = cv_stats(a, d);
    const float mean0 = st[0], g0 = st[1] * a.w0[0], b0 = a.b0[0];
    for (int p = threadIdx.x; p < 2 * a.k; p += 256) {
        float v = (cv_pixel(a, e, r, gr, d, p) - mean0) * g0 + b0;
        if constexpr (TRAIN) v *= cv_factor(a, 0, p, gr);
        img[p] = v;
    }
    __syncthreads();
    for (int ch = wave; ch < kCvCh; ch += 4) {
        float w[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) w[i] = a.cw[ch * 9 + i];
        const float bias = a.cb[ch];
        float* __restrict__ dst = conv + gr * a.F + (int64_t)ch * a.P;
        float s = 0.0f;
        for (int pos = lane; pos < a.P; pos += 64) {
            const int oy = pos / a.OW, ox = pos - oy * a.OW;
            const float* __restrict__ ip = &img[oy * a.W + ox];
            float v = bias;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) v += w[3 * dy + dx] * ip[dy * a.W + dx];
            dst[pos] = v;
            s += v;
        }
        if constexpr (TRAIN) {
            const float mean = wave_sum_xor(s) / (float)a.P;
            float m2 = 0.0f;
            for (int pos = lane; pos < a.P; pos += 64) { const float v = dst[pos] - mean; m2 += v * v; }   // (written by this lane above)
            m2 = wave_sum_xor(m2);
            if (lane == 0) part[gr * kCvCh + ch] = make_float2(mean, m2);
        }
    }
}

// A[row][f] = relu(bn1(conv)) * m1, formed from the stored conv output
template <bool TRAIN>
__device__ __forceinline__ float cv_feature(const CvArgs& a, const float* __restrict__ st, const float* __restrict__ conv, int64_t gr, int f) {
    const int ch = f / a.P;
    float v = fmaxf((conv[gr * a.F + f] - st[2 + ch]) * (st[34 + ch] * a.w1[ch]) + a.b1[ch], 0.0f);
    if constexpr (TRAIN) v *= cv_factor(a, 1, ch, gr);
    return v;
}

// upart[split][row][j] = sum over the split's f of A[row][f] fc_w[j][f].  grid (dirs x row tiles, tiles of 64 j, splits of F): wave w
// owns columns 16 (4 blockIdx.y + w) + l; the A tile of 64 rows x 128 f is staged in LDS in the layout read_blocks<4> reads.
template <bool TRAIN>
__global__ void __launch_bounds__(256) k_conve_fc(CvArgs a, const float* __restrict__ conv, int tiles, int f_per, float* __restrict__ upart) {
    __shared__ float As[kCvKC * kCvStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int d = (int)blockIdx.x / tiles;
    const int64_t b0 = (int64_t)((int)blockIdx.x % tiles) * kCvRows, gr0 = (int64_t)d * a.n + b0;
    const float* __restrict__ st = cv_stats(a, d);
    const int j = 16 * ((int)blockIdx.y * 4 + wave) + l, jc = min(j, a.k - 1);
    const int f_lo = (int)blockIdx.z * f_per, f_hi = min(a.F, f_lo + f_per);
    const float* __restrict__ wp = a.fcw + (int64_t)jc * a.F;
    f32x4v acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int fc0 = f_lo; fc0 < f_hi; fc0 += kCvKC) {
        const int kn = min(kCvKC, f_hi - fc0), kn4 = (kn + 3) & ~3;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kCvKC * kCvRows; idx += 256) {
            const int kl = idx & (kCvKC - 1), rl = idx >> 7;   // consecutive threads: consecutive f of one row
            if (kl >= kn4) continue;
            float v = 0.0f;
            if (b0 + rl < a.n && kl < kn) v = cv_feature<TRAIN>(a, st, conv, gr0 + rl, fc0 + kl);
            As[kl * kCvStride + 4 * (rl & 15) + (rl >> 4)] = v;
        }
        __syncthreads();
        for (int s = 0; s < kn4; s += 4) {
            const float b = wp[min(fc0 + s + g, a.F - 1)];   // (rows of As beyond the chunk are zero)
            float av[4];
            read_blocks<4>(&As[(s + g) * kCvStride], l, av);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], b, acc[mb], 0, 0, 0);
        }
    }
    if (j >= a.k) return;
    float* __restrict__ dst = upart + (int64_t)blockIdx.z * a.n * a.dirs * a.k;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = b0 + 16 * mb + 4 * g + q;
            if (b < a.n) dst[((int64_t)d * a.n + b) * a.k + j] = acc[mb][q];
        }
}

// one wave per column j: u = fc_b + the partial tiles in split order (kept for the backward); training form: the column's bn2
// statistics per direction over u * m2 (tail first, running buffers updated), x = relu(bn2(u * m2)); eval form: x = relu(u)
template <bool TRAIN>
__global__ void __launch_bounds__(256) k_conve_fc_finish(CvArgs a, const float* __restrict__ upart, int splits, float eps, float mom,
                                                         float* __restrict__ run_mean, float* __restrict__ run_var, float* __restrict__ u,
                                                         float* __restrict__ x) {
    const int lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.k) return;
    const int64_t N = a.n * a.dirs;
    const float bias = a.fcb[j];
    for (int d = 0; d < a.dirs; ++d) {
        float s = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            float v = bias;
            for (int sp = 0; sp < splits; ++sp) v += upart[((int64_t)sp * N + gr) * a.k + j];
            if constexpr (TRAIN) {
                u[gr * a.k + j] = v;
                s += v * cv_factor(a, 2, j, gr);
            } else {
                x[gr * a.k + j] = fmaxf(v, 0.0f);
            }
        }
        if constexpr (TRAIN) {
            const float mean = wave_sum_xor(s) / (float)a.n;
            float m2 = 0.0f;
            for (int64_t b = lane; b < a.n; b += 64) {
                const int64_t gr = (int64_t)d * a.n + b;
                const float dv = u[gr * a.k + j] * cv_factor(a, 2, j, gr) - mean;   // (u: written by this lane above)
                m2 += dv * dv;
            }
            m2 = wave_sum_xor(m2);
            const float rstd = 1.0f / sqrtf(m2 / (float)a.n + eps);
            if (lane == 0) {
                float* st = a.stats + (size_t)d * (66 + 2 * a.k);
                st[66 + j] = mean;
                st[66 + a.k + j] = rstd;
                run_mean[j] = (1.0f - mom) * run_mean[j] + mom * mean;
                run_var[j] = (1.0f - mom) * run_var[j] + mom * (m2 / ((float)a.n - 1.0f));
            }
            const float gj = rstd * a.w2[j], bj = a.b2[j];
            for (int64_t b = lane; b < a.n; b += 64) {
                const int64_t gr = (int64_t)d * a.n + b;
                x[gr * a.k + j] = fmaxf((u[gr * a.k + j] * cv_factor(a, 2, j, gr) - mean) * gj + bj, 0.0f);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// one wave per column j, the directions in order: dy2 = dx [bn2 > 0]; S1 = sum dy2, S2 = sum dy2 xh2; du = w2 rstd (dy2 - S1 / n - xh2 S2 / n) m2
__global__ void __launch_bounds__(256) k_conve_bn2_bwd(CvArgs a, const float* __restrict__ dx, const float* __restrict__ u, float* __restrict__ du,
                                                       float* __restrict__ g_w2, float* __restrict__ g_b2, float* __restrict__ g_fcb) {
    const int lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.k) return;
    const float w2 = a.w2[j], b2 = a.b2[j];
    for (int d = 0; d < a.dirs; ++d) {
        const float* __restrict__ st = cv_stats(a, d);
        const float mean = st[66 + j], rstd = st[66 + a.k + j];
        float s1 = 0.0f, s2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            const float xh = (u[gr * a.k + j] * cv_factor(a, 2, j, gr) - mean) * rstd;
            const float dy = xh * w2 + b2 > 0.0f ? dx[gr * a.k + j] : 0.0f;
            s1 += dy;
            s2 += dy * xh;
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        const float inv = 1.0f / (float)a.n;
        float sb = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            const float m = cv_factor(a, 2, j, gr);
            const float xh = (u[gr * a.k + j] * m - mean) * rstd;
            const float dy = xh * w2 + b2 > 0.0f ? dx[gr * a.k + j] : 0.0f;
            const float v = (w2 * rstd) * (dy - s1 * inv - xh * (s2 * inv)) * m;
            du[gr * a.k + j] = v;
            sb += v;
        }
        sb = wave_sum_xor(sb);
        if (lane == 0) { g_w2[j] += s2; g_b2[j] += s1; g_fcb[j] += sb; }
    }
}

// g_fc[j][f] += sum over ALL rows (both directions, in row order) of du[row][j] A[row][f].  grid (ceil(F / 64), ceil(k / 128)): wave w
// owns the 16 f of block 4 blockIdx.x + w for the 128 j of blockIdx.y (8 accumulator blocks); the batch is the contraction.
__global__ void __launch_bounds__(256) k_conve_fc_gw(CvArgs a, const float* __restrict__ conv, const float* __restrict__ du, float* __restrict__ g_fc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int f = 16 * ((int)blockIdx.x * 4 + wave) + l;
    if (f - l >= a.F) return;   // (wave-uniform; F is a multiple of 32, so a live block has all 16 columns)
    const int k0 = (int)blockIdx.y * 128;
    const int nkb = min(8, (a.k - k0 + 15) / 16);
    const int64_t N = a.n * a.dirs;
    f32x4v acc[8];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) acc[kb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t r0 = 0; r0 < N; r0 += 4) {
        const int64_t gr = r0 + g;
        const bool ok = gr < N;
        const int64_t grc = ok ? gr : N - 1;
        const float A = ok ? cv_feature<true>(a, cv_stats(a, (int)(grc / a.n)), conv, grc, f) : 0.0f;
        const float* __restrict__ dp = du + grc * a.k;
#pragma unroll
        for (int kb = 0; kb < 8; ++kb)
            if (kb < nkb) {
                const int j = k0 + 16 * kb + l;
                const float v = ok && j < a.k ? dp[j] : 0.0f;
                acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, A, acc[kb], 0, 0, 0);
            }
    }
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = k0 + 16 * kb + 4 * g + q;
            if (kb < nkb && j < a.k) g_fc[(int64_t)j * a.F + f] += acc[kb][q];
        }
}

// dy1[row][f] = (sum_j du[row][j] fc_w[j][f]) * m1 * [bn1 > 0].  grid (dirs x row tiles, ceil(F / 64)): wave w owns the 16 f of block
// 4 blockIdx.y + w for the tile's 64 rows; the du tile (64 rows x 128 j) is staged in LDS as the forward's A tile is.
__global__ void __launch_bounds__(256) k_conve_fc_da(CvArgs a, const float* __restrict__ conv, const float* __restrict__ du, int tiles,
                                                     float* __restrict__ dy1) {
    __shared__ float As[kCvKC * kCvStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int d = (int)blockIdx.x / tiles;
    const int64_t b0 = (int64_t)((int)blockIdx.x % tiles) * kCvRows, gr0 = (int64_t)d * a.n + b0;
    const int f = 16 * ((int)blockIdx.y * 4 + wave) + l;
    const bool live = f - l < a.F;   // (wave-uniform)
    const int fcl = min(f, a.F - 1);
    f32x4v acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int j0 = 0; j0 < a.k; j0 += kCvKC) {
        const int kn = min(kCvKC, a.k - j0), kn4 = (kn + 3) & ~3;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kCvKC * kCvRows; idx += 256) {
            const int kl = idx & (kCvKC - 1), rl = idx >> 7;
            if (kl >= kn4) continue;
            float v = 0.0f;
            if (b0 + rl < a.n && kl < kn) v = du[(gr0 + rl) * a.k + j0 + kl];
            As[kl * kCvStride + 4 * (rl & 15) + (rl >> 4)] = v;
        }
        __syncthreads();
        if (live)
            for (int s = 0; s < kn4; s += 4) {
                const float b = a.fcw[(int64_t)min(j0 + s + g, a.k - 1) * a.F + fcl];   // (rows of As beyond the chunk are zero)
                float av[4];
                read_blocks<4>(&As[(s + g) * kCvStride], l, av);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], b, acc[mb], 0, 0, 0);
            }
    }
    if (!live) return;
    const float* __restrict__ st = cv_stats(a, d);
    const int ch = f / a.P;
    const float mean = st[2 + ch], gain = st[34 + ch] * a.w1[ch], bias = a.b1[ch];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = b0 + 16 * mb + 4 * g + q;
            if (b >= a.n) continue;
            const int64_t gr = (int64_t)d * a.n + b;
            const float y1 = (conv[gr * a.F + f] - mean) * gain + bias;
            dy1[gr * a.F + f] = y1 > 0.0f ? acc[mb][q] * cv_factor(a, 1, ch, gr) : 0.0f;
        }
}

// one wave per (row, channel): S1 = sum dy1, S2 = sum dy1 xh1 over the row's OH * OW outputs
__global__ void __launch_bounds__(256) k_conve_bn1_part(CvArgs a, const float* __restrict__ conv, const float* __restrict__ dy1, float2* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    const float* __restrict__ st = cv_stats(a, (int)(gr / a.n));
    for (int ch = wave; ch < kCvCh; ch += 4) {
        const float mean = st[2 + ch], rstd = st[34 + ch];
        const int64_t base = gr * a.F + (int64_t)ch * a.P;
        float s1 = 0.0f, s2 = 0.0f;
        for (int pos = lane; pos < a.P; pos += 64) {
            const float dy = dy1[base + pos];
            s1 += dy;
            s2 += dy * ((conv[base + pos] - mean) * rstd);
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        if (lane == 0) part[gr * kCvCh + ch] = make_float2(s1, s2);
    }
}

// one wave per channel, the directions in order: the two sums over the direction's rows -> sums[d][32], g_bn1
__global__ void __launch_bounds__(256) k_conve_bn1_bwd_fin(CvArgs a, const float2* __restrict__ part, float2* __restrict__ sums, float* __restrict__ g_w1,
                                                           float* __restrict__ g_b1) {
    const int lane = threadIdx.x & 63;
    const int ch = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ch >= kCvCh) return;
    for (int d = 0; d < a.dirs; ++d) {
        float s1 = 0.0f, s2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const float2 v = part[((int64_t)d * a.n + b) * kCvCh + ch];
            s1 += v.x;
            s2 += v.y;
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        if (lane == 0) { sums[d * kCvCh + ch] = make_float2(s1, s2); g_w1[ch] += s2; g_b1[ch] += s1; }
    }
}

// one workgroup per row.  Four channels at a time (one per wave): dc = w1 rstd1 (dy1 - S1 / N1 - xh1 S2 / N1) into LDS with the channel's
// 9 filter sums and its bias sum (-> pcw[row][32][10]); then every thread adds the four channels' transposed convolution to its pixels.
// dy0 = that sum * m0 -> dy0[row][2k]; (sum dy0, sum dy0 xh0) of the row -> pt0[row]
__global__ void __launch_bounds__(256) k_conve_conv_bwd(CvArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r, const float* __restrict__ conv,
                                                        const float* __restrict__ dy1, const float2* __restrict__ sums, float* __restrict__ pcw,
                                                        float* __restrict__ dy0, float2* __restrict__ pt0) {
    __shared__ float img[2 * kCvMaxK];       // y0 = bn0(img) * m0, what the convolution read
    __shared__ float dcs[4][2 * kCvMaxK];    // dc of the four channels in flight (OH * OW < 2k)
    __shared__ float accs[2 * kCvMaxK];      // the transposed convolution's sum per pixel
    __shared__ float cws[kCvCh * 9];
    __shared__ float red[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    const int d = (int)(gr / a.n), np = 2 * a.k;
    const float* __restrict__ st = cv_stats(a, d);
    const float mean0 = st[0], rstd0 = st[1], g0 = rstd0 * a.w0[0], b0 = a.b0[0];
    for (int p = threadIdx.x; p < np; p += 256) img[p] = ((cv_pixel(a, e, r, gr, d, p) - mean0) * g0 + b0) * cv_factor(a, 0, p, gr);
    for (int i = threadIdx.x; i < kCvCh * 9; i += 256) cws[i] = a.cw[i];
    const float invN1 = 1.0f / ((float)a.n * (float)a.P);
    const int OH = a.P / a.OW;
    for (int c0 = 0; c0 < kCvCh; c0 += 4) {
        __syncthreads();   // (first pass: img and cws are complete; later: the previous four channels have been consumed)
        {
            const int ch = c0 + wave;
            const float mean = st[2 + ch], rstd = st[34 + ch], gain = a.w1[ch] * rstd;
            const float2 S = sums[d * kCvCh + ch];
            const int64_t base = gr * a.F + (int64_t)ch * a.P;
            float s[10];
#pragma unroll
            for (int i = 0; i < 10; ++i) s[i] = 0.0f;
            for (int pos = lane; pos < a.P; pos += 64) {
                const float xh = (conv[base + pos] - mean) * rstd;
                const float dc = gain * (dy1[base + pos] - S.x * invN1 - xh * (S.y * invN1));
                dcs[wave][pos] = dc;
                const int oy = pos / a.OW, ox = pos - oy * a.OW;
                const float* __restrict__ ip = &img[oy * a.W + ox];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) s[3 * dy + dx] += dc * ip[dy * a.W + dx];
                s[9] += dc;
            }
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const float v = wave_sum_xor(s[i]);
                if (lane == 0) pcw[(gr * kCvCh + ch) * 10 + i] = v;
            }
        }
        __syncthreads();
        for (int p = threadIdx.x; p < np; p += 256) {   // (a thread owns its pixels: accs[p] is read and written by it alone)
            const int y = p / a.W, x = p - y * a.W;
            float v = c0 ? accs[p] : 0.0f;
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const int oy = y - dy;
                    if (oy < 0 || oy >= OH) continue;
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int ox = x - dx;
                        if (ox >= 0 && ox < a.OW) v += dcs[w][oy * a.OW + ox] * cws[(c0 + w) * 9 + 3 * dy + dx];
                    }
                }
            accs[p] = v;
        }
    }
    float t1 = 0.0f, t2 = 0.0f;
    for (int p = threadIdx.x; p < np; p += 256) {
        const float v = accs[p] * cv_factor(a, 0, p, gr);
        dy0[gr * np + p] = v;
        t1 += v;
        t2 += v * ((cv_pixel(a, e, r, gr, d, p) - mean0) * rstd0);
    }
    t1 = wave_sum_xor(t1);
    t2 = wave_sum_xor(t2);
    if (lane == 0) { red[wave] = t1; red[4 + wave] = t2; }
    __syncthreads();
    if (threadIdx.x == 0) pt0[gr] = make_float2(((red[0] + red[1]) + red[2]) + red[3], ((red[4] + red[5]) + red[6]) + red[7]);
}

// waves 0 .. 319: g_conv_w[ch][9] / g_conv_b[ch] += the rows' shares in row order; wave 320: bn0's two sums per direction -> t0[d], g_bn0
__global__ void __launch_bounds__(256) k_conve_small_fin(CvArgs a, const float* __restrict__ pcw, const float2* __restrict__ pt0, float2* __restrict__ t0,
                                                         float* __restrict__ g_cw, float* __restrict__ g_cb, float* __restrict__ g_w0,
                                                         float* __restrict__ g_b0) {
    const int lane = threadIdx.x & 63;
    const int task = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t N = a.n * a.dirs;
    if (task < kCvCh * 10) {
        float s = 0.0f;
        for (int64_t b = lane; b < N; b += 64) s += pcw[b * (kCvCh * 10) + task];
        s = wave_sum_xor(s);
        const int ch = task / 10, i = task - 10 * ch;
        if (lane == 0) { if (i < 9) g_cw[ch * 9 + i] += s; else g_cb[ch] += s; }
    } else if (task == kCvCh * 10) {
        for (int d = 0; d < a.dirs; ++d) {
            float s1 = 0.0f, s2 = 0.0f;
            for (int64_t b = lane; b < a.n; b += 64) { const float2 v = pt0[(int64_t)d * a.n + b]; s1 += v.x; s2 += v.y; }
            s1 = wave_sum_xor(s1);
            s2 = wave_sum_xor(s2);
            if (lane == 0) { t0[d] = make_float2(s1, s2); g_w0[0] += s2; g_b0[0] += s1; }
        }
    }
}

// one wave per row: dy0 -> d loss / d img through bn0, in place; the row's relation row id -> rp
__global__ void __launch_bounds__(256) k_conve_dimg(CvArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r, const float2* __restrict__ t0,
                                                    float* __restrict__ dy0, int64_t* __restrict__ rp) {
    const int lane = threadIdx.x & 63;
    const int64_t gr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gr >= a.n * a.dirs) return;
    const int d = (int)(gr / a.n), np = 2 * a.k;
    const float* __restrict__ st = cv_stats(a, d);
    const float mean0 = st[0], rstd0 = st[1], gain = a.w0[0] * rstd0;
    const float2 T = t0[d];
    const float inv = 1.0f / ((float)a.n * (float)np);
    for (int p = lane; p < np; p += 64) {
        const float xh = (cv_pixel(a, e, r, gr, d, p) - mean0) * rstd0;
        dy0[gr * np + p] = gain * (dy0[gr * np + p] - T.x * inv - xh * (T.y * inv));
    }
    if (lane == 0) rp[gr] = r[gr] + (int64_t)(a.side0 + d) * a.R;
}

// dst[ids[b]][0 .. width) += src[b * stride .. + width) for every row b, in row order and without atomics: the wave of the FIRST row
// that names an id owns that id, walks the later rows 64 at a time (ballot) and adds their shares in order
__global__ void __launch_bounds__(256) k_conve_scatter(const int64_t* __restrict__ ids, int64_t n, int width, const float* __restrict__ src, int stride,
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
                if (c < width) sum += src[s * stride + c];
            }
        }
        if (c < width) dst[id * width + c] += sum;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
struct CvShape {
    int k, h1, H, W, OH, OW, P, F;
};
static CvShape cv_shape(const kge_conve_desc* d) {
    CvShape s{};
    s.k = d->hidden_size; s.h1 = d->hidden_size_1;
    s.H = 2 * (s.k / s.h1); s.W = s.h1; s.OH = s.H - 2; s.OW = s.W - 2; s.P = s.OH * s.OW; s.F = kCvCh * s.P;
    return s;
}

static int cv_check(const kge_conve_desc* d, const char* who, bool grads) {
    if (!d) { set_error("%s: null descriptor", who); return -1; }
    const void* t[] = {d->ent, d->rel, d->b, d->bn0_w, d->bn0_b, d->conv_w, d->conv_b, d->bn1_w, d->bn1_b, d->fc_w, d->fc_b, d->bn2_w, d->bn2_b,
                       d->bn0_mean, d->bn0_var, d->bn1_mean, d->bn1_var, d->bn2_mean, d->bn2_var};
    for (const void* p : t)
        if (!p) { set_error("%s: null tables (the 13 parameters and the six running buffers are all required)", who); return -1; }
    if (d->tot_entity <= 0 || d->tot_relation <= 0 || d->hidden_size <= 0 || d->hidden_size_1 <= 0) {
        set_error("%s: tot_entity, tot_relation, hidden_size and hidden_size_1 must be positive (got %lld, %lld, %d, %d)", who,
                  (long long)d->tot_entity, (long long)d->tot_relation, d->hidden_size, d->hidden_size_1);
        return -1;
    }
    if (d->hidden_size % d->hidden_size_1 != 0) {
        set_error("%s: hidden_size = %d is no multiple of hidden_size_1 = %d (the embedding does not fill the image)", who, d->hidden_size,
                  d->hidden_size_1);
        return -1;
    }
    if (d->hidden_size_1 < 3 || 2 * (d->hidden_size / d->hidden_size_1) < 3) {
        set_error("%s: the image is %d x %d: smaller than the 3 x 3 filter", who, 2 * (d->hidden_size / d->hidden_size_1), d->hidden_size_1);
        return -1;
    }
    if (d->hidden_size > kCvMaxK) { set_error("%s: hidden_size = %d exceeds %d (the image is held in LDS)", who, d->hidden_size, kCvMaxK); return -1; }
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
        const void* g[] = {d->g_ent, d->g_rel, d->g_b, d->g_bn0_w, d->g_bn0_b, d->g_conv_w, d->g_conv_b, d->g_bn1_w, d->g_bn1_b, d->g_fc_w, d->g_fc_b,
                           d->g_bn2_w, d->g_bn2_b};
        for (const void* q : g)
            if (!q) { set_error("%s: null gradient buffers (all 13 are required)", who); return -1; }
    }
    return 0;
}
// rows per direction of a call in training form
static int cv_check_rows(const kge_conve_desc* d, const char* who, int64_t n) {
    if (d->train && n == 1) {
        set_error("%s: batch norm in training form needs more than one row per direction (got n = 1)", who);
        return -1;
    }
    return 0;
}

static CvArgs cv_args(const kge_conve_desc* d, int64_t n, int dirs, int side0, int64_t row0, float* stats) {
    const CvShape s = cv_shape(d);
    CvArgs a{};
    a.ent = d->ent; a.rel = d->rel; a.w0 = d->bn0_w; a.b0 = d->bn0_b; a.cw = d->conv_w; a.cb = d->conv_b; a.w1 = d->bn1_w; a.b1 = d->bn1_b;
    a.fcw = d->fc_w; a.fcb = d->fc_b; a.w2 = d->bn2_w; a.b2 = d->bn2_b;
    a.k = s.k; a.W = s.W; a.P = s.P; a.OW = s.OW; a.F = s.F;
    a.dirs = dirs; a.side0 = side0; a.n = n; a.R = d->tot_relation; a.row0 = (uint32_t)row0;
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

static int cv_tiles(int64_t n) { return (int)((n + kCvRows - 1) / kCvRows); }
// f handled by one workgroup of the fc forward: enough workgroups to fill the device, a function of the shapes alone (the split order
// is the summation order); a multiple of 4
static int cv_f_per(const CvShape& s, int64_t n, int dirs) {
    const int64_t base = (int64_t)dirs * cv_tiles(n) * ((s.k + 63) / 64);
    int64_t splits = (512 + base - 1) / base;
    if (splits > 64) splits = 64;
    if (splits < 1) splits = 1;
    int per = (int)((s.F + splits - 1) / splits);
    per = (per + 3) & ~3;
    return per < 4 ? 4 : per;
}
static int cv_splits(const CvShape& s, int per) { return (s.F + per - 1) / per; }

// saved (floats): conv [N, F] | u [N, k] | stats [dirs][66 + 2k]
static size_t cv_saved_floats(const kge_conve_desc* d, int64_t n, int dirs) {
    const CvShape s = cv_shape(d);
    return (size_t)dirs * ((size_t)n * ((size_t)s.F + s.k) + 66 + 2 * (size_t)s.k);
}
// forward: row partials float2 [N, 32] | upart [splits, N, k]
static size_t cv_fwd_bytes(const kge_conve_desc* d, int64_t n, int dirs) {
    const CvShape s = cv_shape(d);
    const size_t N = (size_t)n * dirs;
    return align256(N * kCvCh * sizeof(float2)) + align256((size_t)cv_splits(s, cv_f_per(s, n, dirs)) * N * s.k * sizeof(float));
}
// backward: du [N, k] | dy1 [N, F] | part1 float2 [N, 32] | sums float2 [dirs, 32] | pcw [N, 320] | dy0 [N, 2k] | pt0 float2 [N] | t0 float2 [dirs] | rp int64 [N]
struct CvBwdPlan {
    size_t du, dy1, part1, sums, pcw, dy0, pt0, t0, rp, total;
};
static CvBwdPlan cv_bwd_plan(const kge_conve_desc* d, int64_t n, int dirs) {
    const CvShape s = cv_shape(d);
    const size_t N = (size_t)n * dirs;
    CvBwdPlan p{};
    p.du = 0;
    p.dy1 = p.du + align256(N * s.k * sizeof(float));
    p.part1 = p.dy1 + align256(N * s.F * sizeof(float));
    p.sums = p.part1 + align256(N * kCvCh * sizeof(float2));
    p.pcw = p.sums + align256((size_t)dirs * kCvCh * sizeof(float2));
    p.dy0 = p.pcw + align256(N * kCvCh * 10 * sizeof(float));
    p.pt0 = p.dy0 + align256(N * 2 * s.k * sizeof(float));
    p.t0 = p.pt0 + align256(N * sizeof(float2));
    p.rp = p.t0 + align256((size_t)dirs * sizeof(float2));
    p.total = p.rp + align256(N * sizeof(int64_t));
    return p;
}

static int cv_forward(const kge_conve_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int side0, int64_t row0, float* x,
                      float* saved, void* ws, hipStream_t st) {
    const CvShape s = cv_shape(d);
    const int64_t N = n * dirs;
    float *conv = saved, *u = conv + N * s.F, *stats = u + N * s.k;
    const CvArgs a = cv_args(d, n, dirs, side0, row0, stats);
    float2* part = (float2*)ws;
    float* upart = (float*)((char*)ws + align256((size_t)N * kCvCh * sizeof(float2)));
    const unsigned row_blocks = (unsigned)((N + 3) / 4);
    const bool train = d->train != 0;
    if (train) {
        hipLaunchKernelGGL(k_conve_img_stats, dim3(row_blocks), dim3(256), 0, st, a, e, r, part);
        hipLaunchKernelGGL(k_conve_bn_fin, dim3(1), dim3(256), 0, st, a, part, 1, 2 * s.k, 0, 1, d->eps[0], d->momentum[0], d->bn0_mean, d->bn0_var);
        hipLaunchKernelGGL((k_conve_conv<true>), dim3((unsigned)N), dim3(256), 0, st, a, e, r, conv, part);
        if (int rc = check_launch("k_conve_img_stats / k_conve_bn_fin / k_conve_conv")) return rc;
        hipLaunchKernelGGL(k_conve_bn_fin, dim3(kCvCh / 4), dim3(256), 0, st, a, part, kCvCh, s.P, 2, 34, d->eps[1], d->momentum[1], d->bn1_mean,
                           d->bn1_var);
    } else {
        hipLaunchKernelGGL(k_conve_stats_eval, dim3(1), dim3(64), 0, st, a, d->eps[0], d->eps[1], d->bn0_mean, d->bn0_var, d->bn1_mean, d->bn1_var);
        hipLaunchKernelGGL((k_conve_conv<false>), dim3((unsigned)N), dim3(256), 0, st, a, e, r, conv, part);
    }
    const int per = cv_f_per(s, n, dirs), splits = cv_splits(s, per), tiles = cv_tiles(n);
    const dim3 grid((unsigned)(dirs * tiles), (unsigned)((s.k + 63) / 64), (unsigned)splits);
    const unsigned col_blocks = (unsigned)((s.k + 3) / 4);
    if (train) {
        hipLaunchKernelGGL((k_conve_fc<true>), grid, dim3(256), 0, st, a, conv, tiles, per, upart);
        hipLaunchKernelGGL((k_conve_fc_finish<true>), dim3(col_blocks), dim3(256), 0, st, a, upart, splits, d->eps[2], d->momentum[2], d->bn2_mean,
                           d->bn2_var, u, x);
    } else {
        hipLaunchKernelGGL((k_conve_fc<false>), grid, dim3(256), 0, st, a, conv, tiles, per, upart);
        hipLaunchKernelGGL((k_conve_fc_finish<false>), dim3(col_blocks), dim3(256), 0, st, a, upart, splits, d->eps[2], d->momentum[2], d->bn2_mean,
                           d->bn2_var, u, x);
    }
    return check_launch("k_conve_fc / k_conve_fc_finish");
}

static int cv_backward(const kge_conve_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int side0, int64_t row0, const float* dx,
                       const float* saved, void* ws, hipStream_t st) {
    const CvShape s = cv_shape(d);
    const int64_t N = n * dirs;
    const float *conv = saved, *u = conv + N * s.F;
    const CvArgs a = cv_args(d, n, dirs, side0, row0, const_cast<float*>(u + N * s.k));
    const CvBwdPlan p = cv_bwd_plan(d, n, dirs);
    char* w = (char*)ws;
    float *du = (float*)(w + p.du), *dy1 = (float*)(w + p.dy1), *pcw = (float*)(w + p.pcw), *dy0 = (float*)(w + p.dy0);
    float2 *part1 = (float2*)(w + p.part1), *sums = (float2*)(w + p.sums), *pt0 = (float2*)(w + p.pt0), *t0 = (float2*)(w + p.t0);
    int64_t* rp = (int64_t*)(w + p.rp);
    const unsigned row_blocks = (unsigned)((N + 3) / 4), col_blocks = (unsigned)((s.k + 3) / 4);
    const int tiles = cv_tiles(n);
    hipLaunchKernelGGL(k_conve_bn2_bwd, dim3(col_blocks), dim3(256), 0, st, a, dx, u, du, d->g_bn2_w, d->g_bn2_b, d->g_fc_b);
    hipLaunchKernelGGL(k_conve_fc_gw, dim3((unsigned)((s.F + 63) / 64), (unsigned)((s.k + 127) / 128)), dim3(256), 0, st, a, conv, du, d->g_fc_w);
    hipLaunchKernelGGL(k_conve_fc_da, dim3((unsigned)(dirs * tiles), (unsigned)((s.F + 63) / 64)), dim3(256), 0, st, a, conv, du, tiles, dy1);
    if (int rc = check_launch("k_conve_bn2_bwd / k_conve_fc_gw / k_conve_fc_da")) return rc;
    hipLaunchKernelGGL(k_conve_bn1_part, dim3((unsigned)N), dim3(256), 0, st, a, conv, dy1, part1);
    hipLaunchKernelGGL(k_conve_bn1_bwd_fin, dim3(kCvCh / 4), dim3(256), 0, st, a, part1, sums, d->g_bn1_w, d->g_bn1_b);
    hipLaunchKernelGGL(k_conve_conv_bwd, dim3((unsigned)N), dim3(256), 0, st, a, e, r, conv, dy1, sums, pcw, dy0, pt0);
    if (int rc = check_launch("k_conve_bn1_part / k_conve_bn1_bwd_fin / k_conve_conv_bwd")) return rc;
    hipLaunchKernelGGL(k_conve_small_fin, dim3((kCvCh * 10 + 1 + 3) / 4), dim3(256), 0, st, a, pcw, pt0, t0, d->g_conv_w, d->g_conv_b, d->g_bn0_w,
                       d->g_bn0_b);
    hipLaunchKernelGGL(k_conve_dimg, dim3(row_blocks), dim3(256), 0, st, a, e, r, t0, dy0, rp);
    hipLaunchKernelGGL(k_conve_scatter, dim3(row_blocks), dim3(256), 0, st, e, N, s.k, dy0, 2 * s.k, d->g_ent);
    hipLaunchKernelGGL(k_conve_scatter, dim3(row_blocks), dim3(256), 0, st, rp, N, s.k, dy0 + s.k, 2 * s.k, d->g_rel);
    return check_launch("k_conve_small_fin / k_conve_dimg / k_conve_scatter");
}

// the relation ids of a call are below tot_relation; the rows read are r + side * tot_relation of a [2R, k] table
static int cv_check_ids(const char* who, const kge_conve_desc* d, const int64_t* e, const int64_t* r, int64_t n, hipStream_t s) {
    return check_er_ids(who, d->tot_entity, d->tot_relation, e, r, n, s);
}

// fused step: ids [4B int64] | x [2B, k] | dx [2B, k] | saved | max(forward, backward, head)
struct CvStepPlan {
    size_t ids, x, dx, saved, rest, total;
};
static CvStepPlan cv_step_plan(const kge_conve_desc* d, int64_t B, int64_t n_hr, int64_t n_tr) {
    CvStepPlan p{};
    const size_t xb = align256((size_t)2 * B * d->hidden_size * sizeof(float));
    p.ids = 0;
    p.x = align256((size_t)4 * B * sizeof(int64_t));
    p.dx = p.x + xb;
    p.saved = p.dx + xb;
    p.rest = p.saved + align256(cv_saved_floats(d, B, 2) * sizeof(float));
    size_t rest = cv_fwd_bytes(d, B, 2);
    if (cv_bwd_plan(d, B, 2).total > rest) rest = cv_bwd_plan(d, B, 2).total;
    const size_t h1 = kge_head_1n_bce_workspace_bytes(B, d->tot_entity, n_hr), h2 = kge_head_1n_bce_workspace_bytes(B, d->tot_entity, n_tr);
    if (h1 > rest) rest = h1;
    if (h2 > rest) rest = h2;
    p.total = p.rest + align256(rest);
    return p;
}

// the rank pass's body (kge_projection.hip): the eval form on the rows [h; t] as two directions; ws = saved | the forward's workspace
static int cv_eval_body(const void* desc, const int64_t* e, const int64_t* r, int64_t n, float* x, void* ws, size_t, hipStream_t s) {
    kge_conve_desc ev = *(const kge_conve_desc*)desc;
    ev.train = 0;
    const size_t saved = align256(cv_saved_floats(&ev, n, 2) * sizeof(float));
    return cv_forward(&ev, e, r, n, 2, 0, 0, x, (float*)ws, (char*)ws + saved, s);
}
static ProjectionEval cv_eval(const kge_conve_desc* d, int64_t n) {
    const int64_t rows = n > 0 ? n : 1;
    return ProjectionEval{d->hidden_size, d->tot_entity, d->tot_relation, d->ent,
                          align256(cv_saved_floats(d, rows, 2) * sizeof(float)) + cv_fwd_bytes(d, rows, 2), cv_eval_body, d->b};
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_conve_saved_floats(const kge_conve_desc* d, int64_t n) {
    return cv_check(d, "kge_conve_saved_floats", false) || n < 0 ? 0 : cv_saved_floats(d, n > 0 ? n : 1, 1);
}

size_t kge_conve_body_forward_workspace_bytes(const kge_conve_desc* d, int64_t n) {
    return cv_check(d, "kge_conve_body_forward_workspace_bytes", false) || n < 0 ? 0 : cv_fwd_bytes(d, n > 0 ? n : 1, 1);
}

int kge_conve_body_forward(const kge_conve_desc* d, const int64_t* e, const int64_t* r, int64_t n, int32_t side, int64_t row0, float* x,
                           float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_conve_body_forward";
    if (cv_check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!e || !r || !x || !saved)) || (side != 0 && side != 1) || row0 < 0 || row0 + n > 0xffffffffLL) {
        set_error("%s: bad arguments (side must be 0 or 1, row0 + n below 2^32)", who);
        return -1;
    }
    if (cv_check_rows(d, who, n)) return -1;
    if (ws_check(who, workspace, workspace_bytes, cv_fwd_bytes(d, n > 0 ? n : 1, 1))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = cv_check_ids(who, d, e, r, n, s)) return rc;
    return cv_forward(d, e, r, n, 1, side, row0, x, saved, workspace, s);
}

size_t kge_conve_body_backward_workspace_bytes(const kge_conve_desc* d, int64_t n) {
    return cv_check(d, "kge_conve_body_backward_workspace_bytes", false) || n < 0 ? 0 : cv_bwd_plan(d, n > 0 ? n : 1, 1).total;
}

int kge_conve_body_backward(const kge_conve_desc* d, const int64_t* e, const int64_t* r, int64_t n, int32_t side, int64_t row0, const float* dx,
                            const float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_conve_body_backward";
    if (cv_check(d, who, true)) return -1;
    if (n < 0 || (n > 0 && (!e || !r || !dx || !saved)) || (side != 0 && side != 1) || row0 < 0 || row0 + n > 0xffffffffLL) {
        set_error("%s: bad arguments (side must be 0 or 1, row0 + n below 2^32)", who);
        return -1;
    }
    if (!d->train) { set_error("%s: the eval form (train = 0) has no backward", who); return -1; }
    if (cv_check_rows(d, who, n)) return -1;
    if (ws_check(who, workspace, workspace_bytes, cv_bwd_plan(d, n > 0 ? n : 1, 1).total)) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = cv_check_ids(who, d, e, r, n, s)) return rc;
    return cv_backward(d, e, r, n, 1, side, row0, dx, saved, workspace, s);
}

size_t kge_conve_train_bce_workspace_bytes(const kge_conve_desc* d, int64_t batch, int64_t n_hr, int64_t n_tr) {
    if (cv_check(d, "kge_conve_train_bce_workspace_bytes", false) || batch < 0 || n_hr < 0 || n_tr < 0) return 0;
    return cv_step_plan(d, batch > 0 ? batch : 1, n_hr, n_tr).total;
}

int kge_conve_train_bce(const kge_conve_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t batch, const int64_t* hr_off,
                        const int32_t* hr_ids, int64_t n_hr, const int64_t* tr_off, const int32_t* tr_ids, int64_t n_tr, float label_smoothing,
                        void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    const char* who = "kge_conve_train_bce";
    if (cv_check(d, who, true)) return -1;
    if (batch < 0 || n_hr < 0 || n_tr < 0 || !loss || (batch > 0 && (!h || !r || !t || !hr_off || !tr_off)) || (n_hr > 0 && !hr_ids) ||
        (n_tr > 0 && !tr_ids) || 2 * batch > 0xffffffffLL) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    if (!d->train) { set_error("%s: the step is the training form (train = 0 has no backward)", who); return -1; }
    if (cv_check_rows(d, who, batch)) return -1;
    const CvStepPlan p = cv_step_plan(d, batch > 0 ? batch : 1, n_hr, n_tr);
    if (ws_check(who, workspace, workspace_bytes, p.total)) return -1;
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t B = batch, n = 2 * B;
    const int k = d->hidden_size;
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
    if (int rc = cv_check_ids(who, d, e, rr, n, s)) return rc;
    // tail direction = forward(h, r, "tail") on rows 0 .. B-1, head direction = forward(t, r, "head") on rows B .. 2B-1, in the same launches
    if (int rc = cv_forward(d, e, rr, B, 2, 0, 0, x, saved, rest, s)) return rc;
    if (int rc = kge_head_1n_bce(x, B, k, d->ent, d->tot_entity, d->b, hr_off, hr_ids, n_hr, label_smoothing, rest, rest_bytes, loss, dx, d->g_ent,
                                 d->g_b, stream)) return rc;
    if (int rc = kge_head_1n_bce(x + B * k, B, k, d->ent, d->tot_entity, d->b, tr_off, tr_ids, n_tr, label_smoothing, rest, rest_bytes, loss,
                                 dx + B * k, d->g_ent, d->g_b, stream)) return rc;
    return cv_backward(d, e, rr, B, 2, 0, 0, dx, saved, rest, s);
}

size_t kge_conve_eval_ranks_workspace_bytes(const kge_conve_desc* d, int64_t n) {
    return cv_check(d, "kge_conve_eval_ranks_workspace_bytes", false) || n < 0 ? 0 : projection_eval_workspace_bytes(cv_eval(d, n), n);
}

int kge_conve_eval_ranks(const kge_conve_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                         const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks, int32_t* ties,
                         void* stream) {
    const char* who = "kge_conve_eval_ranks";
    if (cv_check(d, who, false)) return -1;
    return projection_eval_ranks(who, cv_eval(d, n), d, triples, n, tail_off, tail_ids, head_off, head_ids, workspace, workspace_bytes, ranks,
                                 ties, stream);
}

}  // extern "C"
