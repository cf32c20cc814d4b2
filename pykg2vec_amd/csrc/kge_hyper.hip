// kge_hyper.hip -- the body of HypER (models/projection.py:508-618) in front of the 1-N head of kge_head.hip.
// For a row with entity e and relation r, D = ent_hidden_size, Dr = rel_hidden_size, L = D - 8, F = 32 L:
//     y0   = bn0(ent[e]) * m0                                    one channel over the n D entity values; input dropout, site 0
//     filt = fc1_w rel[r] + fc1_b                                [32 channels][9 taps] PER ROW (k_hyper_filt, VALU); STORED in `saved`
//     c[ch, p] = sum_w y0[p + w] filt[ch, w]                     p in [0, L), no bias; VALU from the row in LDS (k_hyper_conv); STORED once
//     A    = bn1(c) * m1                                         NO relu; feature-map dropout, site 1: a whole channel of a row; never stored
//     u    = A fc_w^T + fc_b                                     [n, F] x [F, D] on v_mfma_f32_16x16x4_f32, F split over workgroups
//                                                                (k_hyper_fc), the partial tiles added in split order (k_hyper_fc_finish)
//     x    = relu(bn2(u * m2))                                   hidden dropout, site 2; bn2 in BOTH forms (eval: running statistics)
// There is one relation table [R, Dr]; a direction selects nothing.  Training form: every batch norm normalises with the statistics
// of ITS DIRECTION's n rows and updates its running buffers, the tail direction first.  Statistics are fixed-order sums: per-row
// (mean, M2) partials over equal counts, combined over the rows in index order with the equal-count form of Chan's rule, as
// kge_conve.hip does.  Eval form (template parameter TRAIN = false): running statistics in bn0, bn1 and bn2, no draws, no writes.
//
// A call works on `dirs` directions of n rows each (body entry points: 1; fused step and rank pass: 2) in the SAME launches: row
// d n + b belongs to direction d.
//
// Backward (training form only), dx the gradient at x:
//     k_hyper_bn2_bwd     du = d loss / d u through relu, bn2 and m2; g_bn2, g_fc_b
//     k_hyper_fc_gw       g_fc[j, f] += sum_b du[b, j] A[b, f]     du^T x A on the matrix cores, ONE owner per output tile walking all rows in order
//     k_hyper_fc_da       dy1 = (du x fc_w) * m1                   du x fc_w on the matrix cores, contraction over D
//     k_hyper_bn1_part / k_hyper_bn1_bwd_fin                       the two sums of bn1's backward, g_bn1
//     k_hyper_conv_bwd    per row: dc from dy1, dfilt[row, ch, w] = sum_p dc[ch, p] y0[p + w], the transposed convolution into dy0
//     k_hyper_small_fin   g_fc1_b[q] = sum_rows dfilt[row, q] and bn0's two sums with g_bn0, over the rows in index order
//     k_hyper_fc1_gw      g_fc1_w[q, i] += sum_rows dfilt[row, q] rel[r_row, i], one thread per element walking all rows in order
//     k_hyper_drel        drel[row] = dfilt[row] . fc1_w (two rows per workgroup)
//     k_hyper_dent        through bn0 to the entity row; k_hyper_scatter adds the rows to g_ent[e] / g_rel[r] in row order (no atomics:
//                         the wave of the FIRST row that names an id owns it) and SKIPS id 0 on both tables (padding_idx = 0)
// No kernel of this file uses atomics.
//
// The dropout draw is the shared one (kge_projection.h spells the Philox counters out), with
//     site 0: elem = pixel in [0, D);   site 1: elem = channel in [0, 32), one draw per row and channel;   site 2: elem = j in [0, D)
//     row = row0 + position in the call's row list.  The fused step numbers the h rows 0 .. B-1 and the t rows B .. 2B-1.
#include "kge_projection.h"
#include "kge_mfma_blocks.h"

namespace kge {

constexpr int kHyMaxK = KGE_HYPER_MAX_HIDDEN;   // both hidden sizes: eight relation rows (k_hyper_filt), the row and four channels of dc (k_hyper_conv_bwd) in LDS
constexpr int kHyCh = 32;           // output channels of the per-row filter
constexpr int kHyTaps = 9;          // filter width
constexpr int kHyQ = kHyCh * kHyTaps;   // fc1's outputs
constexpr int kHyRows = 64;         // batch rows of a matrix-core tile: four 16-row blocks
constexpr int kHyKC = 128;          // contraction elements staged in LDS at a time
constexpr int kHyStride = 68;       // LDS row stride of the staged tile: 16-byte aligned rows, consecutive rows 4 banks apart
constexpr int kHyFR = 8;            // rows of a workgroup in k_hyper_filt
constexpr int kHyQS = 8;            // k_hyper_filt: workgroups that share the 288 outputs of a row group (36 each)
constexpr int kHyDR = 2;            // rows of a workgroup in k_hyper_drel

struct HyArgs {
    const float *ent, *rel, *w0, *b0, *w1, *b1, *w2, *b2, *fcw, *fcb, *f1w, *f1b;
    int D, Dr, L, F;
    int dirs;
    int64_t n;                      // rows per direction
    uint32_t row0;
    int on[3];                      // site draws (training form and p > 0)
    DropKey key;
    uint32_t thr[3];
    float scale[3];
    float* stats;                   // [dirs][66 + 2D]: mean0, rstd0, mean1[32], rstd1[32], mean2[D], rstd2[D]
};
__device__ __forceinline__ const float* hy_stats(const HyArgs& a, int d) { return a.stats + (size_t)d * (66 + 2 * a.D); }
__device__ __forceinline__ float hy_factor(const HyArgs& a, int site, int elem, int64_t gr) {
    return a.on[site] ? drop_row_factor(a.key, site, elem, (int64_t)a.row0 + gr, a.thr[site], a.scale[site]) : 1.0f;
}

// one wave per row: (mean, M2) of the row's D entity values
__global__ void __launch_bounds__(256) k_hyper_row_stats(HyArgs a, const int64_t* __restrict__ e, float2* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t gr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gr >= a.n * a.dirs) return;
    const float* __restrict__ src = a.ent + e[gr] * a.D;
    float s = 0.0f;
    for (int p = lane; p < a.D; p += 64) s += src[p];
    const float mean = wave_sum_xor(s) / (float)a.D;
    float m2 = 0.0f;
    for (int p = lane; p < a.D; p += 64) { const float v = src[p] - mean; m2 += v * v; }
    m2 = wave_sum_xor(m2);
    if (lane == 0) part[gr] = make_float2(mean, m2);
}

// one wave per channel: the statistics of every direction from the per-row partials part[row][chans] (each over cnt values), the tail
// direction first; mean / rstd -> stats, running buffers updated (momentum, unbiased variance)
__global__ void __launch_bounds__(256) k_hyper_bn_fin(HyArgs a, const float2* __restrict__ part, int chans, int cnt, int mean_at, int rstd_at,
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
            float* st = a.stats + (size_t)d * (66 + 2 * a.D);
            st[mean_at + c] = mean;
            st[rstd_at + c] = 1.0f / sqrtf(m2 / tot + eps);
            run_mean[c] = (1.0f - mom) * run_mean[c] + mom * mean;
            run_var[c] = (1.0f - mom) * run_var[c] + mom * (m2 / (tot - 1.0f));
        }
    }
}

// eval form: bn0, bn1 and bn2 normalise with the running buffers
__global__ void __launch_bounds__(256) k_hyper_stats_eval(HyArgs a, float eps0, float eps1, float eps2, const float* __restrict__ rm0,
                                                          const float* __restrict__ rv0, const float* __restrict__ rm1, const float* __restrict__ rv1,
                                                          const float* __restrict__ rm2, const float* __restrict__ rv2) {
    for (int d = 0; d < a.dirs; ++d) {
        float* st = a.stats + (size_t)d * (66 + 2 * a.D);
        for (int t = threadIdx.x; t < 33 + a.D; t += 256) {
            if (t == kHyCh) { st[0] = rm0[0]; st[1] = 1.0f / sqrtf(rv0[0] + eps0); }
            else if (t < kHyCh) { st[2 + t] = rm1[t]; st[34 + t] = 1.0f / sqrtf(rv1[t] + eps1); }
            else { const int j = t - 33; st[66 + j] = rm2[j]; st[66 + a.D + j] = 1.0f / sqrtf(rv2[j] + eps2); }
        }
    }
}

// filt[row][q] = fc1_b[q] + sum_i fc1_w[q][i] rel[r_row][i].  grid (row groups of eight, 8): a workgroup holds the eight relation rows
// in LDS and owns 36 of the 288 q; wave w takes q = q0 + w, q0 + w + 4, ...: its lanes walk i (consecutive floats of fc1_w's row q),
// one wave sum per row
__global__ void __launch_bounds__(256) k_hyper_filt(HyArgs a, const int64_t* __restrict__ r, int64_t N, float* __restrict__ filt) {
    __shared__ float rels[kHyFR][kHyMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kHyFR;
    for (int rr = 0; rr < kHyFR; ++rr) {
        const int64_t gr = min(r0 + rr, N - 1);
        const float* __restrict__ src = a.rel + r[gr] * a.Dr;
        for (int i = threadIdx.x; i < a.Dr; i += 256) rels[rr][i] = src[i];
    }
    __syncthreads();
    const int q0 = (int)blockIdx.y * (kHyQ / kHyQS);
    for (int q = q0 + wave; q < q0 + kHyQ / kHyQS; q += 4) {
        const float* __restrict__ wq = a.f1w + (int64_t)q * a.Dr;
        float acc[kHyFR];
#pragma unroll
        for (int rr = 0; rr < kHyFR; ++rr) acc[rr] = 0.0f;
        for (int i = lane; i < a.Dr; i += 64) {
            const float w = wq[i];
#pragma unroll
            for (int rr = 0; rr < kHyFR; ++rr) acc[rr] += w * rels[rr][i];
        }
        const float bias = a.f1b[q];
#pragma unroll
        for (int rr = 0; rr < kHyFR; ++rr) {
            const float v = wave_sum_xor(acc[rr]) + bias;
            if (lane == 0 && r0 + rr < N) filt[(r0 + rr) * kHyQ + q] = v;
        }
    }
}

// one workgroup per row: y0 = bn0(ent[e]) * m0 and the row's filter into LDS, then one wave per channel: c[ch, p] = sum_w y0[p + w]
// filt[ch, w] -> conv[row][F], and (training form) the channel's (mean, M2) over the row's L outputs -> part[row][32]
template <bool TRAIN>
__global__ void __launch_bounds__(256) k_hyper_conv(HyArgs a, const int64_t* __restrict__ e, const float* __restrict__ filt, float* __restrict__ conv,
                                                    float2* __restrict__ part) {
    __shared__ float img[kHyMaxK];
    __shared__ float fl[kHyQ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    const int d = (int)(gr / a.n);
    const float* __restrict__ st = hy_stats(a, d);
    const float mean0 = st[0], g0 = st[1] * a.w0[0], b0 = a.b0[0];
    const float* __restrict__ src = a.ent + e[gr] * a.D;
    for (int p = threadIdx.x; p < a.D; p += 256) {
        float v = (src[p] - mean0) * g0 + b0;
        if constexpr (TRAIN) v *= hy_factor(a, 0, p, gr);
        img[p] = v;
    }
    for (int q = threadIdx.x; q < kHyQ; q += 256) fl[q] = filt[gr * kHyQ + q];
    __syncthreads();
    for (int ch = wave; ch < kHyCh; ch += 4) {
        float w[kHyTaps];
#pragma unroll
        for (int i = 0; i < kHyTaps; ++i) w[i] = fl[ch * kHyTaps + i];
        float* __restrict__ dst = conv + gr * a.F + (int64_t)ch * a.L;
        float s = 0.0f;
        for (int pos = lane; pos < a.L; pos += 64) {
            float v = 0.0f;
#pragma unroll
            for (int i = 0; i < kHyTaps; ++i) v += w[i] * img[pos + i];
            dst[pos] = v;
            s += v;
        }
        if constexpr (TRAIN) {
            const float mean = wave_sum_xor(s) / (float)a.L;
            float m2 = 0.0f;
            for (int pos = lane; pos < a.L; pos += 64) { const float v = dst[pos] - mean; m2 += v * v; }   // (written by this lane above)
            m2 = wave_sum_xor(m2);
            if (lane == 0) part[gr * kHyCh + ch] = make_float2(mean, m2);
        }
    }
}

// A[row][f] = bn1(conv) * m1, formed from the stored conv output (no relu)
template <bool TRAIN>
__device__ __forceinline__ float hy_feature(const HyArgs& a, const float* __restrict__ st, const float* __restrict__ conv, int64_t gr, int f) {
    const int ch = f / a.L;
    float v = (conv[gr * a.F + f] - st[2 + ch]) * (st[34 + ch] * a.w1[ch]) + a.b1[ch];
    if constexpr (TRAIN) v *= hy_factor(a, 1, ch, gr);
    return v;
}

// upart[split][row][j] = sum over the split's f of A[row][f] fc_w[j][f].  grid (dirs x row tiles, tiles of 64 j, splits of F): wave w
// owns columns 16 (4 blockIdx.y + w) + l; the A tile of 64 rows x 128 f is staged in LDS in the layout read_blocks<4> reads.
template <bool TRAIN>
__global__ void __launch_bounds__(256) k_hyper_fc(HyArgs a, const float* __restrict__ conv, int tiles, int f_per, float* __restrict__ upart) {
    __shared__ float As[kHyKC * kHyStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int d = (int)blockIdx.x / tiles;
    const int64_t b0 = (int64_t)((int)blockIdx.x % tiles) * kHyRows, gr0 = (int64_t)d * a.n + b0;
    const float* __restrict__ st = hy_stats(a, d);
    const int j = 16 * ((int)blockIdx.y * 4 + wave) + l, jc = min(j, a.D - 1);
    const int f_lo = (int)blockIdx.z * f_per, f_hi = min(a.F, f_lo + f_per);
    const float* __restrict__ wp = a.fcw + (int64_t)jc * a.F;
    f32x4v acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int fc0 = f_lo; fc0 < f_hi; fc0 += kHyKC) {
        const int kn = min(kHyKC, f_hi - fc0), kn4 = (kn + 3) & ~3;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kHyKC * kHyRows; idx += 256) {
            const int kl = idx & (kHyKC - 1), rl = idx >> 7;   // consecutive threads: consecutive f of one row
            if (kl >= kn4) continue;
            float v = 0.0f;
            if (b0 + rl < a.n && kl < kn) v = hy_feature<TRAIN>(a, st, conv, gr0 + rl, fc0 + kl);
            As[kl * kHyStride + 4 * (rl & 15) + (rl >> 4)] = v;
        }
        __syncthreads();
        for (int s = 0; s < kn4; s += 4) {
            const float b = wp[min(fc0 + s + g, a.F - 1)];   // (rows of As beyond the chunk are zero)
            float av[4];
            read_blocks<4>(&As[(s + g) * kHyStride], l, av);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], b, acc[mb], 0, 0, 0);
        }
    }
    if (j >= a.D) return;
    float* __restrict__ dst = upart + (int64_t)blockIdx.z * a.n * a.dirs * a.D;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = b0 + 16 * mb + 4 * g + q;
            if (b < a.n) dst[((int64_t)d * a.n + b) * a.D + j] = acc[mb][q];
        }
}

// one wave per column j: u = fc_b + the partial tiles in split order (kept for the backward); training form: the column's bn2
// statistics per direction over u * m2 (tail first, running buffers updated); x = relu(bn2(u * m2)), in the eval form with the
// running statistics k_hyper_stats_eval left in `stats`
template <bool TRAIN>
__global__ void __launch_bounds__(256) k_hyper_fc_finish(HyArgs a, const float* __restrict__ upart, int splits, float eps, float mom,
                                                         float* __restrict__ run_mean, float* __restrict__ run_var, float* __restrict__ u,
                                                         float* __restrict__ x) {
    const int lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.D) return;
    const int64_t N = a.n * a.dirs;
    const float bias = a.fcb[j];
    for (int d = 0; d < a.dirs; ++d) {
        float* st = a.stats + (size_t)d * (66 + 2 * a.D);
        float s = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            float v = bias;
            for (int sp = 0; sp < splits; ++sp) v += upart[((int64_t)sp * N + gr) * a.D + j];
            u[gr * a.D + j] = v;
            if constexpr (TRAIN) s += v * hy_factor(a, 2, j, gr);
        }
        float mean, rstd;
        if constexpr (TRAIN) {
            mean = wave_sum_xor(s) / (float)a.n;
            float m2 = 0.0f;
            for (int64_t b = lane; b < a.n; b += 64) {
                const int64_t gr = (int64_t)d * a.n + b;
                const float dv = u[gr * a.D + j] * hy_factor(a, 2, j, gr) - mean;   // (u: written by this lane above)
                m2 += dv * dv;
            }
            m2 = wave_sum_xor(m2);
            rstd = 1.0f / sqrtf(m2 / (float)a.n + eps);
            if (lane == 0) {
                st[66 + j] = mean;
                st[66 + a.D + j] = rstd;
                run_mean[j] = (1.0f - mom) * run_mean[j] + mom * mean;
                run_var[j] = (1.0f - mom) * run_var[j] + mom * (m2 / ((float)a.n - 1.0f));
            }
        } else {
            mean = st[66 + j];
            rstd = st[66 + a.D + j];
        }
        const float gj = rstd * a.w2[j], bj = a.b2[j];
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            float v = u[gr * a.D + j];
            if constexpr (TRAIN) v *= hy_factor(a, 2, j, gr);
            x[gr * a.D + j] = fmaxf((v - mean) * gj + bj, 0.0f);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// one wave per column j, the directions in order: dy2 = dx [bn2 > 0]; S1 = sum dy2, S2 = sum dy2 xh2; du = w2 rstd (dy2 - S1 / n - xh2 S2 / n) m2
__global__ void __launch_bounds__(256) k_hyper_bn2_bwd(HyArgs a, const float* __restrict__ dx, const float* __restrict__ u, float* __restrict__ du,
                                                       float* __restrict__ g_w2, float* __restrict__ g_b2, float* __restrict__ g_fcb) {
    const int lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.D) return;
    const float w2 = a.w2[j], b2 = a.b2[j];
    for (int d = 0; d < a.dirs; ++d) {
        const float* __restrict__ st = hy_stats(a, d);
        const float mean = st[66 + j], rstd = st[66 + a.D + j];
        float s1 = 0.0f, s2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            const float xh = (u[gr * a.D + j] * hy_factor(a, 2, j, gr) - mean) * rstd;
            const float dy = xh * w2 + b2 > 0.0f ? dx[gr * a.D + j] : 0.0f;
            s1 += dy;
            s2 += dy * xh;
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        const float inv = 1.0f / (float)a.n;
        float sb = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            const float m = hy_factor(a, 2, j, gr);
            const float xh = (u[gr * a.D + j] * m - mean) * rstd;
            const float dy = xh * w2 + b2 > 0.0f ? dx[gr * a.D + j] : 0.0f;
            const float v = (w2 * rstd) * (dy - s1 * inv - xh * (s2 * inv)) * m;
            du[gr * a.D + j] = v;
            sb += v;
        }
        sb = wave_sum_xor(sb);
        if (lane == 0) { g_w2[j] += s2; g_b2[j] += s1; g_fcb[j] += sb; }
    }
}

// g_fc[j][f] += sum over ALL rows (both directions, in row order) of du[row][j] A[row][f].  grid (ceil(F / 64), ceil(D / 128)): wave w
// owns the 16 f of block 4 blockIdx.x + w for the 128 j of blockIdx.y (8 accumulator blocks); the batch is the contraction.
__global__ void __launch_bounds__(256) k_hyper_fc_gw(HyArgs a, const float* __restrict__ conv, const float* __restrict__ du, float* __restrict__ g_fc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int f = 16 * ((int)blockIdx.x * 4 + wave) + l;
    if (f - l >= a.F) return;   // (wave-uniform; F is a multiple of 32, so a live block has all 16 columns)
    const int k0 = (int)blockIdx.y * 128;
    const int nkb = min(8, (a.D - k0 + 15) / 16);
    const int64_t N = a.n * a.dirs;
    f32x4v acc[8];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) acc[kb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t r0 = 0; r0 < N; r0 += 4) {
        const int64_t gr = r0 + g;
        const bool ok = gr < N;
        const int64_t grc = ok ? gr : N - 1;
        const float A = ok ? hy_feature<true>(a, hy_stats(a, (int)(grc / a.n)), conv, grc, f) : 0.0f;
        const float* __restrict__ dp = du + grc * a.D;
#pragma unroll
        for (int kb = 0; kb < 8; ++kb)
            if (kb < nkb) {
                const int j = k0 + 16 * kb + l;
                const float v = ok && j < a.D ? dp[j] : 0.0f;
                acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, A, acc[kb], 0, 0, 0);
            }
    }
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = k0 + 16 * kb + 4 * g + q;
            if (kb < nkb && j < a.D) g_fc[(int64_t)j * a.F + f] += acc[kb][q];
        }
}

// dy1[row][f] = (sum_j du[row][j] fc_w[j][f]) * m1.  grid (dirs x row tiles, ceil(F / 64)): wave w owns the 16 f of block
// 4 blockIdx.y + w for the tile's 64 rows; the du tile (64 rows x 128 j) is staged in LDS as the forward's A tile is.
__global__ void __launch_bounds__(256) k_hyper_fc_da(HyArgs a, const float* __restrict__ du, int tiles, float* __restrict__ dy1) {
    __shared__ float As[kHyKC * kHyStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int d = (int)blockIdx.x / tiles;
    const int64_t b0 = (int64_t)((int)blockIdx.x % tiles) * kHyRows, gr0 = (int64_t)d * a.n + b0;
    const int f = 16 * ((int)blockIdx.y * 4 + wave) + l;
    const bool live = f - l < a.F;   // (wave-uniform)
    const int fcl = min(f, a.F - 1);
    f32x4v acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int j0 = 0; j0 < a.D; j0 += kHyKC) {
        const int kn = min(kHyKC, a.D - j0), kn4 = (kn + 3) & ~3;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kHyKC * kHyRows; idx += 256) {
            const int kl = idx & (kHyKC - 1), rl = idx >> 7;
            if (kl >= kn4) continue;
            float v = 0.0f;
            if (b0 + rl < a.n && kl < kn) v = du[(gr0 + rl) * a.D + j0 + kl];
            As[kl * kHyStride + 4 * (rl & 15) + (rl >> 4)] = v;
        }
        __syncthreads();
        if (live)
            for (int s = 0; s < kn4; s += 4) {
                const float b = a.fcw[(int64_t)min(j0 + s + g, a.D - 1) * a.F + fcl];   // (rows of As beyond the chunk are zero)
                float av[4];
                read_blocks<4>(&As[(s + g) * kHyStride], l, av);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], b, acc[mb], 0, 0, 0);
            }
    }
    if (!live) return;
    const int ch = f / a.L;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = b0 + 16 * mb + 4 * g + q;
            if (b >= a.n) continue;
            const int64_t gr = (int64_t)d * a.n + b;
            dy1[gr * a.F + f] = acc[mb][q] * hy_factor(a, 1, ch, gr);
        }
}

// one wave per (row, channel): S1 = sum dy1, S2 = sum dy1 xh1 over the row's L outputs
__global__ void __launch_bounds__(256) k_hyper_bn1_part(HyArgs a, const float* __restrict__ conv, const float* __restrict__ dy1, float2* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    const float* __restrict__ st = hy_stats(a, (int)(gr / a.n));
    for (int ch = wave; ch < kHyCh; ch += 4) {
        const float mean = st[2 + ch], rstd = st[34 + ch];
        const int64_t base = gr * a.F + (int64_t)ch * a.L;
        float s1 = 0.0f, s2 = 0.0f;
        for (int pos = lane; pos < a.L; pos += 64) {
            const float dy = dy1[base + pos];
            s1 += dy;
            s2 += dy * ((conv[base + pos] - mean) * rstd);
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        if (lane == 0) part[gr * kHyCh + ch] = make_float2(s1, s2);
    }
}

// one wave per channel, the directions in order: the two sums over the direction's rows -> sums[d][32], g_bn1
__global__ void __launch_bounds__(256) k_hyper_bn1_bwd_fin(HyArgs a, const float2* __restrict__ part, float2* __restrict__ sums, float* __restrict__ g_w1,
                                                           float* __restrict__ g_b1) {
    const int lane = threadIdx.x & 63;
    const int ch = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ch >= kHyCh) return;
    for (int d = 0; d < a.dirs; ++d) {
        float s1 = 0.0f, s2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const float2 v = part[((int64_t)d * a.n + b) * kHyCh + ch];
            s1 += v.x;
            s2 += v.y;
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        if (lane == 0) { sums[d * kHyCh + ch] = make_float2(s1, s2); g_w1[ch] += s2; g_b1[ch] += s1; }
    }
}

// one workgroup per row.  Four channels at a time (one per wave): dc = w1 rstd1 (dy1 - S1 / N1 - xh1 S2 / N1) into LDS with the channel's
// nine filter sums dfilt[row][ch][w] = sum_p dc[p] y0[p + w]; then every thread adds the four channels' transposed convolution (with
// the ROW's filter) to its pixels.  dy0 = that sum * m0 -> dy0[row][D]; (sum dy0, sum dy0 xh0) of the row -> pt0[row]
__global__ void __launch_bounds__(256) k_hyper_conv_bwd(HyArgs a, const int64_t* __restrict__ e, const float* __restrict__ filt,
                                                        const float* __restrict__ conv, const float* __restrict__ dy1, const float2* __restrict__ sums,
                                                        float* __restrict__ dfilt, float* __restrict__ dy0, float2* __restrict__ pt0) {
    __shared__ float img[kHyMaxK];       // y0 = bn0(ent[e]) * m0, what the convolution read
    __shared__ float dcs[4][kHyMaxK];    // dc of the four channels in flight (L < D)
    __shared__ float accs[kHyMaxK];      // the transposed convolution's sum per pixel
    __shared__ float fl[kHyQ];
    __shared__ float red[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    const int d = (int)(gr / a.n);
    const float* __restrict__ st = hy_stats(a, d);
    const float mean0 = st[0], rstd0 = st[1], g0 = rstd0 * a.w0[0], b0 = a.b0[0];
    const float* __restrict__ src = a.ent + e[gr] * a.D;
    for (int p = threadIdx.x; p < a.D; p += 256) img[p] = ((src[p] - mean0) * g0 + b0) * hy_factor(a, 0, p, gr);
    for (int q = threadIdx.x; q < kHyQ; q += 256) fl[q] = filt[gr * kHyQ + q];
    const float invN1 = 1.0f / ((float)a.n * (float)a.L);
    for (int c0 = 0; c0 < kHyCh; c0 += 4) {
        __syncthreads();   // (first pass: img and fl are complete; later: the previous four channels have been consumed)
        {
            const int ch = c0 + wave;
            const float mean = st[2 + ch], rstd = st[34 + ch], gain = a.w1[ch] * rstd;
            const float2 S = sums[d * kHyCh + ch];
            const int64_t base = gr * a.F + (int64_t)ch * a.L;
            float s[kHyTaps];
#pragma unroll
            for (int i = 0; i < kHyTaps; ++i) s[i] = 0.0f;
            for (int pos = lane; pos < a.L; pos += 64) {
                const float xh = (conv[base + pos] - mean) * rstd;
                const float dc = gain * (dy1[base + pos] - S.x * invN1 - xh * (S.y * invN1));
                dcs[wave][pos] = dc;
#pragma unroll
                for (int i = 0; i < kHyTaps; ++i) s[i] += dc * img[pos + i];
            }
#pragma unroll
            for (int i = 0; i < kHyTaps; ++i) {
                const float v = wave_sum_xor(s[i]);
                if (lane == 0) dfilt[gr * kHyQ + ch * kHyTaps + i] = v;
            }
        }
        __syncthreads();
        for (int p = threadIdx.x; p < a.D; p += 256) {   // (a thread owns its pixels: accs[p] is read and written by it alone)
            float v = 0.0f;   // (the four channels' 36 terms first, then ONE addition to the running sum: shorter error growth than 288 in a row)
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int i = 0; i < kHyTaps; ++i) {
                    const int pos = p - i;
                    if (pos >= 0 && pos < a.L) v += dcs[w][pos] * fl[(c0 + w) * kHyTaps + i];
                }
            accs[p] = c0 ? accs[p] + v : v;
        }
    }
    float t1 = 0.0f, t2 = 0.0f;
    for (int p = threadIdx.x; p < a.D; p += 256) {
        const float v = accs[p] * hy_factor(a, 0, p, gr);
        dy0[gr * a.D + p] = v;
        t1 += v;
        t2 += v * ((src[p] - mean0) * rstd0);
    }
    t1 = wave_sum_xor(t1);
    t2 = wave_sum_xor(t2);
    if (lane == 0) { red[wave] = t1; red[4 + wave] = t2; }
    __syncthreads();
    if (threadIdx.x == 0) pt0[gr] = make_float2(((red[0] + red[1]) + red[2]) + red[3], ((red[4] + red[5]) + red[6]) + red[7]);
}

// waves 0 .. 287: g_fc1_b[q] += the rows' dfilt[row][q] in row order; wave 288: bn0's two sums per direction -> t0[d], g_bn0
__global__ void __launch_bounds__(256) k_hyper_small_fin(HyArgs a, const float* __restrict__ dfilt, const float2* __restrict__ pt0, float2* __restrict__ t0,
                                                         float* __restrict__ g_f1b, float* __restrict__ g_w0, float* __restrict__ g_b0) {
    const int lane = threadIdx.x & 63;
    const int task = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t N = a.n * a.dirs;
    if (task < kHyQ) {
        float s = 0.0f;
        for (int64_t b = lane; b < N; b += 64) s += dfilt[b * kHyQ + task];
        s = wave_sum_xor(s);
        if (lane == 0) g_f1b[task] += s;
    } else if (task == kHyQ) {
        for (int d = 0; d < a.dirs; ++d) {
            float s1 = 0.0f, s2 = 0.0f;
            for (int64_t b = lane; b < a.n; b += 64) { const float2 v = pt0[(int64_t)d * a.n + b]; s1 += v.x; s2 += v.y; }
            s1 = wave_sum_xor(s1);
            s2 = wave_sum_xor(s2);
            if (lane == 0) { t0[d] = make_float2(s1, s2); g_w0[0] += s2; g_b0[0] += s1; }
        }
    }
}

// g_fc1_w[q][i] += sum over ALL rows, in row order, of dfilt[row][q] rel[r_row][i]: one thread per element (consecutive threads:
// consecutive i of one q)
__global__ void __launch_bounds__(256) k_hyper_fc1_gw(HyArgs a, const int64_t* __restrict__ r, const float* __restrict__ dfilt,
                                                      float* __restrict__ g_f1w) {
    const int t = (int)blockIdx.x * 256 + threadIdx.x;
    if (t >= kHyQ * a.Dr) return;
    const int q = t / a.Dr, i = t - q * a.Dr;
    const int64_t N = a.n * a.dirs;
    float s = 0.0f;
#pragma unroll 8
    for (int64_t b = 0; b < N; ++b) s += dfilt[b * kHyQ + q] * a.rel[r[b] * a.Dr + i];
    g_f1w[t] += s;
}

// drel[row][i] = sum_q dfilt[row][q] fc1_w[q][i], q in order.  One workgroup per two rows (their dfilt rows in LDS); a thread owns i
__global__ void __launch_bounds__(256) k_hyper_drel(HyArgs a, const float* __restrict__ dfilt, int64_t N, float* __restrict__ drel) {
    __shared__ float dfl[kHyDR][kHyQ];
    const int64_t r0 = (int64_t)blockIdx.x * kHyDR;
    for (int idx = threadIdx.x; idx < kHyDR * kHyQ; idx += 256) {
        const int rr = idx / kHyQ, q = idx - rr * kHyQ;
        dfl[rr][q] = r0 + rr < N ? dfilt[(r0 + rr) * kHyQ + q] : 0.0f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.Dr; i += 256) {
        float acc[kHyDR];
#pragma unroll
        for (int rr = 0; rr < kHyDR; ++rr) acc[rr] = 0.0f;
#pragma unroll 8
        for (int q = 0; q < kHyQ; ++q) {
            const float w = a.f1w[(int64_t)q * a.Dr + i];
#pragma unroll
            for (int rr = 0; rr < kHyDR; ++rr) acc[rr] += dfl[rr][q] * w;
        }
#pragma unroll
        for (int rr = 0; rr < kHyDR; ++rr)
            if (r0 + rr < N) drel[(r0 + rr) * a.Dr + i] = acc[rr];
    }
}

// one wave per row: dy0 -> d loss / d ent[e] through bn0, in place
__global__ void __launch_bounds__(256) k_hyper_dent(HyArgs a, const int64_t* __restrict__ e, const float2* __restrict__ t0, float* __restrict__ dy0) {
    const int lane = threadIdx.x & 63;
    const int64_t gr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gr >= a.n * a.dirs) return;
    const int d = (int)(gr / a.n);
    const float* __restrict__ st = hy_stats(a, d);
    const float mean0 = st[0], rstd0 = st[1], gain = a.w0[0] * rstd0;
    const float2 T = t0[d];
    const float inv = 1.0f / ((float)a.n * (float)a.D);
    const float* __restrict__ src = a.ent + e[gr] * a.D;
    for (int p = lane; p < a.D; p += 64) {
        const float xh = (src[p] - mean0) * rstd0;
        dy0[gr * a.D + p] = gain * (dy0[gr * a.D + p] - T.x * inv - xh * (T.y * inv));
    }
}

// dst[ids[b]][0 .. width) += src[b * width .. + width) for every row b with ids[b] != 0 (padding_idx = 0: the lookup's gradient of id 0
// is dropped), in row order and without atomics: the wave of the FIRST row that names an id owns that id, walks the later rows 64 at
// a time (ballot) and adds their shares in order
__global__ void __launch_bounds__(256) k_hyper_scatter(const int64_t* __restrict__ ids, int64_t n, int width, const float* __restrict__ src,
                                                       float* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int64_t id = ids[row];
    if (id == 0) return;   // (wave-uniform)
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
struct HyShape {
    int D, Dr, L, F;
};
static HyShape hy_shape(const kge_hyper_desc* d) {
    HyShape s{};
    s.D = d->ent_hidden_size; s.Dr = d->rel_hidden_size; s.L = s.D - (kHyTaps - 1); s.F = kHyCh * s.L;
    return s;
}

static int hy_check(const kge_hyper_desc* d, const char* who, bool grads) {
    if (!d) { set_error("%s: null descriptor", who); return -1; }
    const void* t[] = {d->b, d->ent, d->rel, d->bn0_w, d->bn0_b, d->bn1_w, d->bn1_b, d->bn2_w, d->bn2_b, d->fc_w, d->fc_b, d->fc1_w, d->fc1_b,
                       d->bn0_mean, d->bn0_var, d->bn1_mean, d->bn1_var, d->bn2_mean, d->bn2_var};
    for (const void* p : t)
        if (!p) { set_error("%s: null tables (the 13 parameters and the six running buffers are all required)", who); return -1; }
    if (d->tot_entity <= 0 || d->tot_relation <= 0 || d->ent_hidden_size <= 0 || d->rel_hidden_size <= 0) {
        set_error("%s: tot_entity, tot_relation, ent_hidden_size and rel_hidden_size must be positive (got %lld, %lld, %d, %d)", who,
                  (long long)d->tot_entity, (long long)d->tot_relation, d->ent_hidden_size, d->rel_hidden_size);
        return -1;
    }
    if (d->ent_hidden_size < kHyTaps) {
        set_error("%s: ent_hidden_size = %d is shorter than the %d-tap filter (no conv output)", who, d->ent_hidden_size, kHyTaps);
        return -1;
    }
    if (d->ent_hidden_size > kHyMaxK || d->rel_hidden_size > kHyMaxK) {
        set_error("%s: ent_hidden_size = %d / rel_hidden_size = %d exceeds %d (the rows are held in LDS)", who, d->ent_hidden_size,
                  d->rel_hidden_size, kHyMaxK);
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
        const void* g[] = {d->g_b, d->g_ent, d->g_rel, d->g_bn0_w, d->g_bn0_b, d->g_bn1_w, d->g_bn1_b, d->g_bn2_w, d->g_bn2_b, d->g_fc_w, d->g_fc_b,
                           d->g_fc1_w, d->g_fc1_b};
        for (const void* q : g)
            if (!q) { set_error("%s: null gradient buffers (all 13 are required)", who); return -1; }
    }
    return 0;
}
// rows per direction of a call in training form
static int hy_check_rows(const kge_hyper_desc* d, const char* who, int64_t n) {
    if (d->train && n == 1) {
        set_error("%s: batch norm in training form needs more than one row per direction (got n = 1)", who);
        return -1;
    }
    return 0;
}

static HyArgs hy_args(const kge_hyper_desc* d, int64_t n, int dirs, int64_t row0, float* stats) {
    const HyShape s = hy_shape(d);
    HyArgs a{};
    a.ent = d->ent; a.rel = d->rel; a.w0 = d->bn0_w; a.b0 = d->bn0_b; a.w1 = d->bn1_w; a.b1 = d->bn1_b; a.w2 = d->bn2_w; a.b2 = d->bn2_b;
    a.fcw = d->fc_w; a.fcb = d->fc_b; a.f1w = d->fc1_w; a.f1b = d->fc1_b;
    a.D = s.D; a.Dr = s.Dr; a.L = s.L; a.F = s.F;
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

static int hy_tiles(int64_t n) { return (int)((n + kHyRows - 1) / kHyRows); }
// f handled by one workgroup of the fc forward: enough workgroups to fill the device, a function of the shapes alone (the split order
// is the summation order); a multiple of 4
static int hy_f_per(const HyShape& s, int64_t n, int dirs) {
    const int64_t base = (int64_t)dirs * hy_tiles(n) * ((s.D + 63) / 64);
    int64_t splits = (512 + base - 1) / base;
    if (splits > 64) splits = 64;
    if (splits < 1) splits = 1;
    int per = (int)((s.F + splits - 1) / splits);
    per = (per + 3) & ~3;
    return per < 4 ? 4 : per;
}
static int hy_splits(const HyShape& s, int per) { return (s.F + per - 1) / per; }

// saved (floats): conv [N, F] | u [N, D] | filt [N, 288] | stats [dirs][66 + 2D]
static size_t hy_saved_floats(const kge_hyper_desc* d, int64_t n, int dirs) {
    const HyShape s = hy_shape(d);
    return (size_t)dirs * ((size_t)n * ((size_t)s.F + s.D + kHyQ) + 66 + 2 * (size_t)s.D);
}
// forward: row partials float2 [N, 32] | upart [splits, N, D]
static size_t hy_fwd_bytes(const kge_hyper_desc* d, int64_t n, int dirs) {
    const HyShape s = hy_shape(d);
    const size_t N = (size_t)n * dirs;
    return align256(N * kHyCh * sizeof(float2)) + align256((size_t)hy_splits(s, hy_f_per(s, n, dirs)) * N * s.D * sizeof(float));
}
// backward: du [N, D] | dy1 [N, F] | part1 float2 [N, 32] | sums float2 [dirs, 32] | dfilt [N, 288] | dy0 [N, D] | drel [N, Dr] | pt0 float2 [N] | t0 float2 [dirs]
struct HyBwdPlan {
    size_t du, dy1, part1, sums, dfilt, dy0, drel, pt0, t0, total;
};
static HyBwdPlan hy_bwd_plan(const kge_hyper_desc* d, int64_t n, int dirs) {
    const HyShape s = hy_shape(d);
    const size_t N = (size_t)n * dirs;
    HyBwdPlan p{};
    p.du = 0;
    p.dy1 = p.du + align256(N * s.D * sizeof(float));
    p.part1 = p.dy1 + align256(N * s.F * sizeof(float));
    p.sums = p.part1 + align256(N * kHyCh * sizeof(float2));
    p.dfilt = p.sums + align256((size_t)dirs * kHyCh * sizeof(float2));
    p.dy0 = p.dfilt + align256(N * kHyQ * sizeof(float));
    p.drel = p.dy0 + align256(N * s.D * sizeof(float));
    p.pt0 = p.drel + align256(N * s.Dr * sizeof(float));
    p.t0 = p.pt0 + align256(N * sizeof(float2));
    p.total = p.t0 + align256((size_t)dirs * sizeof(float2));
    return p;
}

static int hy_forward(const kge_hyper_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int64_t row0, float* x, float* saved,
                      void* ws, hipStream_t st) {
    const HyShape s = hy_shape(d);
    const int64_t N = n * dirs;
    float *conv = saved, *u = conv + N * s.F, *filt = u + N * s.D, *stats = filt + N * kHyQ;
    const HyArgs a = hy_args(d, n, dirs, row0, stats);
    float2* part = (float2*)ws;
    float* upart = (float*)((char*)ws + align256((size_t)N * kHyCh * sizeof(float2)));
    const unsigned row_blocks = (unsigned)((N + 3) / 4);
    const bool train = d->train != 0;
    hipLaunchKernelGGL(k_hyper_filt, dim3((unsigned)((N + kHyFR - 1) / kHyFR), kHyQS), dim3(256), 0, st, a, r, N, filt);
    if (train) {
        hipLaunchKernelGGL(k_hyper_row_stats, dim3(row_blocks), dim3(256), 0, st, a, e, part);
        hipLaunchKernelGGL(k_hyper_bn_fin, dim3(1), dim3(256), 0, st, a, part, 1, s.D, 0, 1, d->eps[0], d->momentum[0], d->bn0_mean, d->bn0_var);
        hipLaunchKernelGGL((k_hyper_conv<true>), dim3((unsigned)N), dim3(256), 0, st, a, e, filt, conv, part);
        if (int rc = check_launch("k_hyper_filt / k_hyper_row_stats / k_hyper_bn_fin / k_hyper_conv")) return rc;
        hipLaunchKernelGGL(k_hyper_bn_fin, dim3(kHyCh / 4), dim3(256), 0, st, a, part, kHyCh, s.L, 2, 34, d->eps[1], d->momentum[1], d->bn1_mean,
                           d->bn1_var);
    } else {
        hipLaunchKernelGGL(k_hyper_stats_eval, dim3(1), dim3(256), 0, st, a, d->eps[0], d->eps[1], d->eps[2], d->bn0_mean, d->bn0_var, d->bn1_mean,
                           d->bn1_var, d->bn2_mean, d->bn2_var);
        hipLaunchKernelGGL((k_hyper_conv<false>), dim3((unsigned)N), dim3(256), 0, st, a, e, filt, conv, part);
    }
    const int per = hy_f_per(s, n, dirs), splits = hy_splits(s, per), tiles = hy_tiles(n);
    const dim3 grid((unsigned)(dirs * tiles), (unsigned)((s.D + 63) / 64), (unsigned)splits);
    const unsigned col_blocks = (unsigned)((s.D + 3) / 4);
    if (train) {
        hipLaunchKernelGGL((k_hyper_fc<true>), grid, dim3(256), 0, st, a, conv, tiles, per, upart);
        hipLaunchKernelGGL((k_hyper_fc_finish<true>), dim3(col_blocks), dim3(256), 0, st, a, upart, splits, d->eps[2], d->momentum[2], d->bn2_mean,
                           d->bn2_var, u, x);
    } else {
        hipLaunchKernelGGL((k_hyper_fc<false>), grid, dim3(256), 0, st, a, conv, tiles, per, upart);
        hipLaunchKernelGGL((k_hyper_fc_finish<false>), dim3(col_blocks), dim3(256), 0, st, a, upart, splits, d->eps[2], d->momentum[2], d->bn2_mean,
                           d->bn2_var, u, x);
    }
    return check_launch("k_hyper_fc / k_hyper_fc_finish");
}

static int hy_backward(const kge_hyper_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int64_t row0, const float* dx,
                       const float* saved, void* ws, hipStream_t st) {
    const HyShape s = hy_shape(d);
    const int64_t N = n * dirs;
    const float *conv = saved, *u = conv + N * s.F, *filt = u + N * s.D;
    const HyArgs a = hy_args(d, n, dirs, row0, const_cast<float*>(filt + N * kHyQ));
    const HyBwdPlan p = hy_bwd_plan(d, n, dirs);
    char* w = (char*)ws;
    float *du = (float*)(w + p.du), *dy1 = (float*)(w + p.dy1), *dfilt = (float*)(w + p.dfilt), *dy0 = (float*)(w + p.dy0), *drel = (float*)(w + p.drel);
    float2 *part1 = (float2*)(w + p.part1), *sums = (float2*)(w + p.sums), *pt0 = (float2*)(w + p.pt0), *t0 = (float2*)(w + p.t0);
    const unsigned row_blocks = (unsigned)((N + 3) / 4), col_blocks = (unsigned)((s.D + 3) / 4);
    const unsigned row2_blocks = (unsigned)((N + kHyDR - 1) / kHyDR);
    const int tiles = hy_tiles(n);
    hipLaunchKernelGGL(k_hyper_bn2_bwd, dim3(col_blocks), dim3(256), 0, st, a, dx, u, du, d->g_bn2_w, d->g_bn2_b, d->g_fc_b);
    hipLaunchKernelGGL(k_hyper_fc_gw, dim3((unsigned)((s.F + 63) / 64), (unsigned)((s.D + 127) / 128)), dim3(256), 0, st, a, conv, du, d->g_fc_w);
    hipLaunchKernelGGL(k_hyper_fc_da, dim3((unsigned)(dirs * tiles), (unsigned)((s.F + 63) / 64)), dim3(256), 0, st, a, du, tiles, dy1);
    if (int rc = check_launch("k_hyper_bn2_bwd / k_hyper_fc_gw / k_hyper_fc_da")) return rc;
    hipLaunchKernelGGL(k_hyper_bn1_part, dim3((unsigned)N), dim3(256), 0, st, a, conv, dy1, part1);
    hipLaunchKernelGGL(k_hyper_bn1_bwd_fin, dim3(kHyCh / 4), dim3(256), 0, st, a, part1, sums, d->g_bn1_w, d->g_bn1_b);
    hipLaunchKernelGGL(k_hyper_conv_bwd, dim3((unsigned)N), dim3(256), 0, st, a, e, filt, conv, dy1, sums, dfilt, dy0, pt0);
    if (int rc = check_launch("k_hyper_bn1_part / k_hyper_bn1_bwd_fin / k_hyper_conv_bwd")) return rc;
    hipLaunchKernelGGL(k_hyper_small_fin, dim3((kHyQ + 1 + 3) / 4), dim3(256), 0, st, a, dfilt, pt0, t0, d->g_fc1_b, d->g_bn0_w, d->g_bn0_b);
    hipLaunchKernelGGL(k_hyper_fc1_gw, dim3((unsigned)((kHyQ * s.Dr + 255) / 256)), dim3(256), 0, st, a, r, dfilt, d->g_fc1_w);
    hipLaunchKernelGGL(k_hyper_drel, dim3(row2_blocks), dim3(256), 0, st, a, dfilt, N, drel);
    hipLaunchKernelGGL(k_hyper_dent, dim3(row_blocks), dim3(256), 0, st, a, e, t0, dy0);
    if (int rc = check_launch("k_hyper_small_fin / k_hyper_fc1_gw / k_hyper_drel / k_hyper_dent")) return rc;
    hipLaunchKernelGGL(k_hyper_scatter, dim3(row_blocks), dim3(256), 0, st, e, N, s.D, dy0, d->g_ent);
    hipLaunchKernelGGL(k_hyper_scatter, dim3(row_blocks), dim3(256), 0, st, r, N, s.Dr, drel, d->g_rel);
    return check_launch("k_hyper_scatter");
}

static int hy_check_ids(const char* who, const kge_hyper_desc* d, const int64_t* e, const int64_t* r, int64_t n, hipStream_t s) {
    return check_er_ids(who, d->tot_entity, d->tot_relation, e, r, n, s);
}

// fused step: ids [4B int64] | x [2B, D] | dx [2B, D] | saved | max(forward, backward, head)
struct HyStepPlan {
    size_t ids, x, dx, saved, rest, total;
};
static HyStepPlan hy_step_plan(const kge_hyper_desc* d, int64_t B, int64_t n_hr, int64_t n_tr) {
    HyStepPlan p{};
    const size_t xb = align256((size_t)2 * B * d->ent_hidden_size * sizeof(float));
    p.ids = 0;
    p.x = align256((size_t)4 * B * sizeof(int64_t));
    p.dx = p.x + xb;
    p.saved = p.dx + xb;
    p.rest = p.saved + align256(hy_saved_floats(d, B, 2) * sizeof(float));
    size_t rest = hy_fwd_bytes(d, B, 2);
    if (hy_bwd_plan(d, B, 2).total > rest) rest = hy_bwd_plan(d, B, 2).total;
    const size_t h1 = kge_head_1n_bce_workspace_bytes(B, d->tot_entity, n_hr), h2 = kge_head_1n_bce_workspace_bytes(B, d->tot_entity, n_tr);
    if (h1 > rest) rest = h1;
    if (h2 > rest) rest = h2;
    p.total = p.rest + align256(rest);
    return p;
}

// the rank pass's body (kge_projection.hip): the eval form on the rows [h; t] as two directions; ws = saved | the forward's workspace
static int hy_eval_body(const void* desc, const int64_t* e, const int64_t* r, int64_t n, float* x, void* ws, size_t, hipStream_t s) {
    kge_hyper_desc ev = *(const kge_hyper_desc*)desc;
    ev.train = 0;
    const size_t saved = align256(hy_saved_floats(&ev, n, 2) * sizeof(float));
    return hy_forward(&ev, e, r, n, 2, 0, x, (float*)ws, (char*)ws + saved, s);
}
static ProjectionEval hy_eval(const kge_hyper_desc* d, int64_t n) {
    const int64_t rows = n > 0 ? n : 1;
    return ProjectionEval{d->ent_hidden_size, d->tot_entity, d->tot_relation, d->ent,
                          align256(hy_saved_floats(d, rows, 2) * sizeof(float)) + hy_fwd_bytes(d, rows, 2), hy_eval_body, d->b};
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_hyper_saved_floats(const kge_hyper_desc* d, int64_t n) {
    return hy_check(d, "kge_hyper_saved_floats", false) || n < 0 ? 0 : hy_saved_floats(d, n > 0 ? n : 1, 1);
}

size_t kge_hyper_body_forward_workspace_bytes(const kge_hyper_desc* d, int64_t n) {
    return hy_check(d, "kge_hyper_body_forward_workspace_bytes", false) || n < 0 ? 0 : hy_fwd_bytes(d, n > 0 ? n : 1, 1);
}

int kge_hyper_body_forward(const kge_hyper_desc* d, const int64_t* e, const int64_t* r, int64_t n, int64_t row0, float* x, float* saved,
                           void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_hyper_body_forward";
    if (hy_check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!e || !r || !x || !saved)) || row0 < 0 || row0 + n > 0xffffffffLL) {
        set_error("%s: bad arguments (row0 + n below 2^32)", who);
        return -1;
    }
    if (hy_check_rows(d, who, n)) return -1;
    if (ws_check(who, workspace, workspace_bytes, hy_fwd_bytes(d, n > 0 ? n : 1, 1))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = hy_check_ids(who, d, e, r, n, s)) return rc;
    return hy_forward(d, e, r, n, 1, row0, x, saved, workspace, s);
}

size_t kge_hyper_body_backward_workspace_bytes(const kge_hyper_desc* d, int64_t n) {
    return hy_check(d, "kge_hyper_body_backward_workspace_bytes", false) || n < 0 ? 0 : hy_bwd_plan(d, n > 0 ? n : 1, 1).total;
}

int kge_hyper_body_backward(const kge_hyper_desc* d, const int64_t* e, const int64_t* r, int64_t n, int64_t row0, const float* dx,
                            const float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_hyper_body_backward";
    if (hy_check(d, who, true)) return -1;
    if (n < 0 || (n > 0 && (!e || !r || !dx || !saved)) || row0 < 0 || row0 + n > 0xffffffffLL) {
        set_error("%s: bad arguments (row0 + n below 2^32)", who);
        return -1;
    }
    if (!d->train) { set_error("%s: the eval form (train = 0) has no backward", who); return -1; }
    if (hy_check_rows(d, who, n)) return -1;
    if (ws_check(who, workspace, workspace_bytes, hy_bwd_plan(d, n > 0 ? n : 1, 1).total)) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = hy_check_ids(who, d, e, r, n, s)) return rc;
    return hy_backward(d, e, r, n, 1, row0, dx, saved, workspace, s);
}

size_t kge_hyper_train_bce_workspace_bytes(const kge_hyper_desc* d, int64_t batch, int64_t n_hr, int64_t n_tr) {
    if (hy_check(d, "kge_hyper_train_bce_workspace_bytes", false) || batch < 0 || n_hr < 0 || n_tr < 0) return 0;
    return hy_step_plan(d, batch > 0 ? batch : 1, n_hr, n_tr).total;
}

int kge_hyper_train_bce(const kge_hyper_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t batch, const int64_t* hr_off,
                        const int32_t* hr_ids, int64_t n_hr, const int64_t* tr_off, const int32_t* tr_ids, int64_t n_tr, float label_smoothing,
                        void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    const char* who = "kge_hyper_train_bce";
    if (hy_check(d, who, true)) return -1;
    if (batch < 0 || n_hr < 0 || n_tr < 0 || !loss || (batch > 0 && (!h || !r || !t || !hr_off || !tr_off)) || (n_hr > 0 && !hr_ids) ||
        (n_tr > 0 && !tr_ids) || 2 * batch > 0xffffffffLL) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    if (!d->train) { set_error("%s: the step is the training form (train = 0 has no backward)", who); return -1; }
    if (hy_check_rows(d, who, batch)) return -1;
    const HyStepPlan p = hy_step_plan(d, batch > 0 ? batch : 1, n_hr, n_tr);
    if (ws_check(who, workspace, workspace_bytes, p.total)) return -1;
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t B = batch, n = 2 * B;
    const int k = d->ent_hidden_size;
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
    if (int rc = hy_check_ids(who, d, e, rr, n, s)) return rc;
    // tail direction = forward(h, r, "tail") on rows 0 .. B-1, head direction = forward(t, r, "head") on rows B .. 2B-1, in the same launches
    if (int rc = hy_forward(d, e, rr, B, 2, 0, x, saved, rest, s)) return rc;
    if (int rc = kge_head_1n_bce(x, B, k, d->ent, d->tot_entity, d->b, hr_off, hr_ids, n_hr, label_smoothing, rest, rest_bytes, loss, dx, d->g_ent,
                                 d->g_b, stream)) return rc;
    if (int rc = kge_head_1n_bce(x + B * k, B, k, d->ent, d->tot_entity, d->b, tr_off, tr_ids, n_tr, label_smoothing, rest, rest_bytes, loss,
                                 dx + B * k, d->g_ent, d->g_b, stream)) return rc;
    return hy_backward(d, e, rr, B, 2, 0, dx, saved, rest, s);
}

size_t kge_hyper_eval_ranks_workspace_bytes(const kge_hyper_desc* d, int64_t n) {
    return hy_check(d, "kge_hyper_eval_ranks_workspace_bytes", false) || n < 0 ? 0 : projection_eval_workspace_bytes(hy_eval(d, n), n);
}

int kge_hyper_eval_ranks(const kge_hyper_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                         const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks, int32_t* ties,
                         void* stream) {
    const char* who = "kge_hyper_eval_ranks";
    if (hy_check(d, who, false)) return -1;
    return projection_eval_ranks(who, hy_eval(d, n), d, triples, n, tail_off, tail_ids, head_off, head_ids, workspace, workspace_bytes, ranks,
                                 ties, stream);
}

}  // extern "C"
