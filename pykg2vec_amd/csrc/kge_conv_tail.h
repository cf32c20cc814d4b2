// kge_conv_tail.h -- the back half that the conv 1-N bodies share (kge_conve.hip, kge_hyper.hip, kge_interacte.hip, kge_acre.hip; DESIGN.md
// section 22).  Behind its own convolution front every one of them computes, from the stored conv output [N, F] of C channels,
//     A    = feature(bn1(conv))                                  the model's: relu or not, feature-map dropout (site 1); never stored
//     u    = A fc_w^T + fc_b                                     [n, F] x [F, K] on v_mfma_f32_16x16x4_f32, F split over workgroups
//                                                                (k_*_fc), the partial tiles added in split order (k_*_fc_finish)
//     x    = relu(bn2(u * m2))                                   hidden dropout, site 2
// and, backward, k_*_bn2_bwd (du, g_bn2, g_fc_b), k_*_fc_gw (g_fc, ONE owner per output tile walking all rows in order),
// k_*_fc_da (dy1, the gradient at bn1's output), k_*_bn1_part / k_*_bn1_bwd_fin (the two sums of bn1's backward, g_bn1) and
// k_*_scatter (the ordered, atomic-free row scatter).  k_*_bn_fin combines the per-row (mean, M2) partials of bn0 and bn1.
//
// A kernel body is a template over the model's policy M, a plain struct of static functions resolved at compile time, and every model
// gets its own named kernels around the bodies (k_conve_fc, k_hyper_fc, ...: KGE_CONV_TAIL_KERNELS below), specialised as before, with the floating-point expressions, summation orders, grids, LDS layout and launch bounds they had as
// separate copies.  The policy supplies
//     Args, Desc                        the kernel argument struct (it names the tail's fields as said below) and the descriptor of include/kge_hip.h
//     K(a), F(a), C(a), E(a)            fc outputs, flat features, channels, values per channel (F = C E)
//     SS(a), o1(a), o2(a)               floats of `stats` per direction; mean1 at o1, rstd1 at o1 + C, mean2 at o2, rstd2 at o2 + K
//     feature<TRAIN>(a, st, conv, m1f, gr, f)        A[gr][f]
//     Bn1, bn1_chan(a, st, ch)                       what dy1 needs of channel ch, read ONCE per thread before k_*_fc_da's stores
//     dy1(a, bn, conv, m1f, gr, f, ch, acc)          what k_*_fc_da stores for the product acc: relu mask and site-1 factor
//     kClamp                            F need not be a multiple of 16: k_*_fc_gw / k_*_fc_da clamp f and mask the lanes beyond F
//     kEvalBn2                          the eval form normalises with bn2's running statistics (ConvE's: x = relu(u))
// and, for the host templates at the end of this file, check / forward / backward, the workspace sizes, dim, the head's bias and the
// argument message kBadArgs.  `side` is ConvE's (which half of its relation table a direction reads); the other bodies ignore it.
#pragma once
#include "kge_projection.h"
#include "kge_mfma_blocks.h"

namespace kge {

constexpr int kTailRows = 64;       // batch rows of a matrix-core tile: four 16-row blocks
constexpr int kTailKC = 128;        // contraction elements staged in LDS at a time
constexpr int kTailStride = 68;     // LDS row stride of the staged tile: 16-byte aligned rows, consecutive rows 4 banks apart

// Every model's Args carries, under these names, what the tail reads: fcw, fcb, w1, b1, w2, b2, dirs, n (rows per direction), row0,
// on[3] (site draws: training form and p > 0), key, thr[3], scale[3], stats ([dirs][SS]).  The field ORDER stays each model's own (the
// kernarg layout of its front kernels is the one they were tuned with).
template <class A>
__device__ __forceinline__ float tail_factor(const A& a, int site, int elem, int64_t gr) {
    return a.on[site] ? drop_row_factor(a.key, site, elem, (int64_t)a.row0 + gr, a.thr[site], a.scale[site]) : 1.0f;
}
template <class M>
__device__ __forceinline__ float* tail_stats(const typename M::Args& a, int d) { return a.stats + (size_t)d * M::SS(a); }

// the device half of the policy of a body that applies a relu and STORES its site-1 factors m1f [N, C] (InteractE, AcrE); its Args
// carry K, HW, C, F and the runtime stats layout SS, o1, o2
template <class A>
struct TailReluM1f {
    using Args = A;
    static constexpr bool kClamp = true, kEvalBn2 = true;
    __host__ __device__ static int K(const Args& a) { return a.K; }
    __host__ __device__ static int F(const Args& a) { return a.F; }
    __host__ __device__ static int C(const Args& a) { return a.C; }
    __host__ __device__ static int E(const Args& a) { return a.HW; }
    __host__ __device__ static int SS(const Args& a) { return a.SS; }
    __host__ __device__ static int o1(const Args& a) { return a.o1; }
    __host__ __device__ static int o2(const Args& a) { return a.o2; }
    // y1 = bn1(conv) before the relu, and A[row][f] = relu(y1) * m1, formed from the stored conv output
    __device__ __forceinline__ static float bn1(const Args& a, const float* __restrict__ st, const float* __restrict__ conv, int64_t gr, int f, int ch) {
        return (conv[gr * a.F + f] - st[a.o1 + ch]) * (st[a.o1 + a.C + ch] * a.w1[ch]) + a.b1[ch];
    }
    template <bool TRAIN>
    __device__ __forceinline__ static float feature(const Args& a, const float* __restrict__ st, const float* __restrict__ conv,
                                                    const float* __restrict__ m1f, int64_t gr, int f) {
        const int ch = f / a.HW;
        float v = fmaxf(bn1(a, st, conv, gr, f, ch), 0.0f);
        if constexpr (TRAIN) v *= m1f[gr * a.C + ch];
        return v;
    }
    struct Bn1 {
        const float* st;
    };
    __device__ __forceinline__ static Bn1 bn1_chan(const Args&, const float* st, int) { return Bn1{st}; }
    __device__ __forceinline__ static float dy1(const Args& a, const Bn1& bn, const float* __restrict__ conv, const float* __restrict__ m1f, int64_t gr,
                                                int f, int ch, float acc) {
        const float keep = bn1(a, bn.st, conv, gr, f, ch) > 0.0f ? m1f[gr * a.C + ch] : 0.0f;
        return acc * keep;
    }
};

// one wave per channel: the statistics of every direction from the per-row partials part[row * pstride + c * pmul] (each over cnt
// values), the tail direction first; mean / rstd -> stats, running buffers updated (momentum, unbiased variance).  One partial per
// row that serves every channel: pstride 1, pmul 0; a partial per row and channel: pstride = chans, pmul 1
template <class M>
__device__ __forceinline__ void tail_bn_fin_body(const typename M::Args& a, const float2* __restrict__ part, int chans, int pstride, int pmul, int cnt,
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
            float* st = tail_stats<M>(a, d);
            st[mean_at + c] = mean;
            st[rstd_at + c] = 1.0f / sqrtf(m2 / tot + eps);
            run_mean[c] = (1.0f - mom) * run_mean[c] + mom * mean;
            run_var[c] = (1.0f - mom) * run_var[c] + mom * (m2 / (tot - 1.0f));
        }
    }
}

// upart[split][row][j] = sum over the split's f of A[row][f] fc_w[j][f].  grid (dirs x row tiles, tiles of 64 j, splits of F): wave w
// owns columns 16 (4 blockIdx.y + w) + l; the A tile of 64 rows x 128 f is staged in LDS in the layout read_blocks<4> reads.
template <class M, bool TRAIN>
__device__ __forceinline__ void tail_fc_body(const typename M::Args& a, const float* __restrict__ conv, const float* __restrict__ m1f, int tiles, int f_per,
                                             float* __restrict__ upart) {
    __shared__ float As[kTailKC * kTailStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int K = M::K(a), F = M::F(a);
    const int d = (int)blockIdx.x / tiles;
    const int64_t b0 = (int64_t)((int)blockIdx.x % tiles) * kTailRows, gr0 = (int64_t)d * a.n + b0;
    const float* __restrict__ st = tail_stats<M>(a, d);
    const int j = 16 * ((int)blockIdx.y * 4 + wave) + l, jc = min(j, K - 1);
    const int f_lo = (int)blockIdx.z * f_per, f_hi = min(F, f_lo + f_per);
    const float* __restrict__ wp = a.fcw + (int64_t)jc * F;
    f32x4v acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int fc0 = f_lo; fc0 < f_hi; fc0 += kTailKC) {
        const int kn = min(kTailKC, f_hi - fc0), kn4 = (kn + 3) & ~3;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kTailKC * kTailRows; idx += 256) {
            const int kl = idx & (kTailKC - 1), rl = idx >> 7;   // consecutive threads: consecutive f of one row
            if (kl >= kn4) continue;
            float v = 0.0f;
            if (b0 + rl < a.n && kl < kn) v = M::template feature<TRAIN>(a, st, conv, m1f, gr0 + rl, fc0 + kl);
            As[kl * kTailStride + 4 * (rl & 15) + (rl >> 4)] = v;
        }
        __syncthreads();
        for (int s = 0; s < kn4; s += 4) {
            const float b = wp[min(fc0 + s + g, F - 1)];   // (rows of As beyond the chunk are zero)
            float av[4];
            read_blocks<4>(&As[(s + g) * kTailStride], l, av);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], b, acc[mb], 0, 0, 0);
        }
    }
    if (j >= K) return;
    float* __restrict__ dst = upart + (int64_t)blockIdx.z * a.n * a.dirs * K;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = b0 + 16 * mb + 4 * g + q;
            if (b < a.n) dst[((int64_t)d * a.n + b) * K + j] = acc[mb][q];
        }
}

// one wave per column j: u = fc_b + the partial tiles in split order (kept for the backward); training form: the column's bn2
// statistics per direction over u * m2 (tail first, running buffers updated); x = relu(bn2(u * m2)), in the eval form with the
// running statistics the model's stats_eval kernel left in `stats` -- or, without kEvalBn2, x = relu(u) and u is not written
template <class M, bool TRAIN>
__device__ __forceinline__ void tail_fc_finish_body(const typename M::Args& a, const float* __restrict__ upart, int splits, float eps, float mom,
                                                    float* __restrict__ run_mean, float* __restrict__ run_var, float* __restrict__ u,
                                                    float* __restrict__ x) {
    constexpr bool BN2 = TRAIN || M::kEvalBn2;
    const int lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int K = M::K(a);
    if (j >= K) return;
    const int64_t N = a.n * a.dirs;
    const float bias = a.fcb[j];
    for (int d = 0; d < a.dirs; ++d) {
        float* st = tail_stats<M>(a, d);
        float s = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            float v = bias;
            for (int sp = 0; sp < splits; ++sp) v += upart[((int64_t)sp * N + gr) * K + j];
            if constexpr (BN2) u[gr * K + j] = v;
            else x[gr * K + j] = fmaxf(v, 0.0f);
            if constexpr (TRAIN) s += v * tail_factor(a, 2, j, gr);
        }
        if constexpr (BN2) {
            float mean, rstd;
            if constexpr (TRAIN) {
                mean = wave_sum_xor(s) / (float)a.n;
                float m2 = 0.0f;
                for (int64_t b = lane; b < a.n; b += 64) {
                    const int64_t gr = (int64_t)d * a.n + b;
                    const float dv = u[gr * K + j] * tail_factor(a, 2, j, gr) - mean;   // (u: written by this lane above)
                    m2 += dv * dv;
                }
                m2 = wave_sum_xor(m2);
                rstd = 1.0f / sqrtf(m2 / (float)a.n + eps);
                if (lane == 0) {
                    st[M::o2(a) + j] = mean;
                    st[M::o2(a) + K + j] = rstd;
                    run_mean[j] = (1.0f - mom) * run_mean[j] + mom * mean;
                    run_var[j] = (1.0f - mom) * run_var[j] + mom * (m2 / ((float)a.n - 1.0f));
                }
            } else {
                mean = st[M::o2(a) + j];
                rstd = st[M::o2(a) + K + j];
            }
            const float gj = rstd * a.w2[j], bj = a.b2[j];
            for (int64_t b = lane; b < a.n; b += 64) {
                const int64_t gr = (int64_t)d * a.n + b;
                float v = u[gr * K + j];
                if constexpr (TRAIN) v *= tail_factor(a, 2, j, gr);
                x[gr * K + j] = fmaxf((v - mean) * gj + bj, 0.0f);
            }
        }
    }
}

// one wave per column j, the directions in order: dy2 = dx [bn2 > 0]; S1 = sum dy2, S2 = sum dy2 xh2; du = w2 rstd (dy2 - S1 / n - xh2 S2 / n) m2
template <class M>
__device__ __forceinline__ void tail_bn2_bwd_body(const typename M::Args& a, const float* __restrict__ dx, const float* __restrict__ u,
                                                  float* __restrict__ du, float* __restrict__ g_w2, float* __restrict__ g_b2,
                                                  float* __restrict__ g_fcb) {
    const int lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int K = M::K(a);
    if (j >= K) return;
    const float w2 = a.w2[j], b2 = a.b2[j];
    for (int d = 0; d < a.dirs; ++d) {
        const float* __restrict__ st = tail_stats<M>(a, d);
        const float mean = st[M::o2(a) + j], rstd = st[M::o2(a) + K + j];
        float s1 = 0.0f, s2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            const float xh = (u[gr * K + j] * tail_factor(a, 2, j, gr) - mean) * rstd;
            const float dy = xh * w2 + b2 > 0.0f ? dx[gr * K + j] : 0.0f;
            s1 += dy;
            s2 += dy * xh;
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        const float inv = 1.0f / (float)a.n;
        float sb = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const int64_t gr = (int64_t)d * a.n + b;
            const float m = tail_factor(a, 2, j, gr);
            const float xh = (u[gr * K + j] * m - mean) * rstd;
            const float dy = xh * w2 + b2 > 0.0f ? dx[gr * K + j] : 0.0f;
            const float v = (w2 * rstd) * (dy - s1 * inv - xh * (s2 * inv)) * m;
            du[gr * K + j] = v;
            sb += v;
        }
        sb = wave_sum_xor(sb);
        if (lane == 0) { g_w2[j] += s2; g_b2[j] += s1; g_fcb[j] += sb; }
    }
}

// g_fc[j][f] += sum over ALL rows (both directions, in row order) of du[row][j] A[row][f].  grid (ceil(F / 64), ceil(K / 128)): wave w
// owns the 16 f of block 4 blockIdx.x + w for the 128 j of blockIdx.y (8 accumulator blocks); the batch is the contraction.  With
// kClamp a lane beyond F contributes zeros and stores nothing; without it F is a multiple of 16 and a live block has all 16 columns.
template <class M>
__device__ __forceinline__ void tail_fc_gw_body(const typename M::Args& a, const float* __restrict__ conv, const float* __restrict__ m1f,
                                                const float* __restrict__ du, float* __restrict__ g_fc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int K = M::K(a), F = M::F(a);
    const int f = 16 * ((int)blockIdx.x * 4 + wave) + l;
    if (f - l >= F) return;   // (wave-uniform)
    const bool fok = !M::kClamp || f < F;
    const int fcl = M::kClamp ? min(f, F - 1) : f;
    const int k0 = (int)blockIdx.y * 128;
    const int nkb = min(8, (K - k0 + 15) / 16);
    const int64_t N = a.n * a.dirs;
    f32x4v acc[8];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) acc[kb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t r0 = 0; r0 < N; r0 += 4) {
        const int64_t gr = r0 + g;
        const bool ok = gr < N;
        const int64_t grc = ok ? gr : N - 1;
        float A;
        if constexpr (M::kClamp) {
            const float v1 = M::template feature<true>(a, tail_stats<M>(a, (int)(grc / a.n)), conv, m1f, grc, fcl);
            A = ok && fok ? v1 : 0.0f;
        } else {
            A = ok ? M::template feature<true>(a, tail_stats<M>(a, (int)(grc / a.n)), conv, m1f, grc, f) : 0.0f;
        }
        const float* __restrict__ dp = du + grc * K;
#pragma unroll
        for (int kb = 0; kb < 8; ++kb)
            if (kb < nkb) {
                const int j = k0 + 16 * kb + l;
                const float v = ok && j < K ? dp[M::kClamp ? min(j, K - 1) : j] : 0.0f;
                acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, A, acc[kb], 0, 0, 0);
            }
    }
    if (!fok) return;
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = k0 + 16 * kb + 4 * g + q;
            if (kb < nkb && j < K) g_fc[(int64_t)j * F + f] += acc[kb][q];
        }
}

// dy1[row][f] = M::dy1(sum_j du[row][j] fc_w[j][f]): the gradient at bn1's output.  grid (dirs x row tiles, ceil(F / 64)): wave w owns
// the 16 f of block 4 blockIdx.y + w for the tile's 64 rows; the du tile (64 rows x 128 j) is staged in LDS as the forward's A tile is.
template <class M>
__device__ __forceinline__ void tail_fc_da_body(const typename M::Args& a, const float* __restrict__ conv, const float* __restrict__ m1f,
                                                const float* __restrict__ du, int tiles, float* __restrict__ dy1) {
    __shared__ float As[kTailKC * kTailStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int K = M::K(a), F = M::F(a);
    const int d = (int)blockIdx.x / tiles;
    const int64_t b0 = (int64_t)((int)blockIdx.x % tiles) * kTailRows, gr0 = (int64_t)d * a.n + b0;
    const float* __restrict__ st = tail_stats<M>(a, d);
    const int f = 16 * ((int)blockIdx.y * 4 + wave) + l;
    const bool live = f - l < F;   // (wave-uniform)
    const int fcl = min(f, F - 1);
    f32x4v acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int j0 = 0; j0 < K; j0 += kTailKC) {
        const int kn = min(kTailKC, K - j0), kn4 = (kn + 3) & ~3;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kTailKC * kTailRows; idx += 256) {
            const int kl = idx & (kTailKC - 1), rl = idx >> 7;
            if (kl >= kn4) continue;
            float v = 0.0f;
            if (b0 + rl < a.n && kl < kn) v = du[(gr0 + rl) * K + j0 + kl];
            As[kl * kTailStride + 4 * (rl & 15) + (rl >> 4)] = v;
        }
        __syncthreads();
        if (live)
            for (int s = 0; s < kn4; s += 4) {
                const float b = a.fcw[(int64_t)min(j0 + s + g, K - 1) * F + fcl];   // (rows of As beyond the chunk are zero)
                float av[4];
                read_blocks<4>(&As[(s + g) * kTailStride], l, av);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], b, acc[mb], 0, 0, 0);
            }
    }
    if (!live || (M::kClamp && f >= F)) return;
    const int ch = f / M::E(a);
    const typename M::Bn1 bn = M::bn1_chan(a, st, ch);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t b = b0 + 16 * mb + 4 * g + q;
            if (b >= a.n) continue;
            const int64_t gr = (int64_t)d * a.n + b;
            dy1[gr * F + f] = M::dy1(a, bn, conv, m1f, gr, f, ch, acc[mb][q]);
        }
}

// one wave per (row, channel), grid (rows, channel groups): S1 = sum dy1, S2 = sum dy1 xh1 over the channel's E outputs of the row
template <class M>
__device__ __forceinline__ void tail_bn1_part_body(const typename M::Args& a, const float* __restrict__ conv, const float* __restrict__ dy1,
                                                   float2* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = M::C(a), E = M::E(a);
    const int64_t gr = blockIdx.x;
    const float* __restrict__ st = tail_stats<M>(a, (int)(gr / a.n));
    for (int ch = (int)blockIdx.y * 4 + wave; ch < C; ch += 4 * (int)gridDim.y) {
        const float mean = st[M::o1(a) + ch], rstd = st[M::o1(a) + C + ch];
        const int64_t base = gr * M::F(a) + (int64_t)ch * E;
        float s1 = 0.0f, s2 = 0.0f;
        for (int pos = lane; pos < E; pos += 64) {
            const float dy = dy1[base + pos];
            s1 += dy;
            s2 += dy * ((conv[base + pos] - mean) * rstd);
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        if (lane == 0) part[gr * C + ch] = make_float2(s1, s2);
    }
}

// one wave per channel, the directions in order: the two sums over the direction's rows -> sums[d][C], g_bn1
template <class M>
__device__ __forceinline__ void tail_bn1_bwd_fin_body(const typename M::Args& a, const float2* __restrict__ part, float2* __restrict__ sums,
                                                      float* __restrict__ g_w1, float* __restrict__ g_b1) {
    const int lane = threadIdx.x & 63;
    const int ch = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int C = M::C(a);
    if (ch >= C) return;
    for (int d = 0; d < a.dirs; ++d) {
        float s1 = 0.0f, s2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) {
            const float2 v = part[((int64_t)d * a.n + b) * C + ch];
            s1 += v.x;
            s2 += v.y;
        }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        if (lane == 0) { sums[d * C + ch] = make_float2(s1, s2); g_w1[ch] += s2; g_b1[ch] += s1; }
    }
}

// dst[ids[b]][0 .. width) += src[b * stride .. + width) for every row b -- with SKIP0 only those with ids[b] != 0 (padding_idx = 0: the
// lookup's gradient of id 0 is dropped) -- in row order and without atomics: the wave of the FIRST row that names an id owns that id,
// walks the later rows 64 at a time (ballot) and adds their shares in order
template <bool SKIP0>
__device__ __forceinline__ void tail_scatter_body(const int64_t* __restrict__ ids, int64_t n, int width, const float* __restrict__ src, int stride,
                                                  float* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int64_t id = ids[row];
    if (SKIP0 && id == 0) return;   // (wave-uniform)
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

// The kernels themselves carry the model's name, as its front kernels do (k_<stem>_fc<TRAIN>, k_<stem>_scatter, ...): named __global__
// shells around the bodies above, one set per model, defined by this macro next to the model's policy M.  TailKernels<M> hands them
// to the host templates below; SKIP0 is the model's scatter rule.
template <class M>
struct TailKernels;
#define KGE_TAIL_KERNEL __global__ void __launch_bounds__(256)
#define KGE_CONV_TAIL_KERNELS(stem, M, SKIP0)                                                                                                     \
    KGE_TAIL_KERNEL k_##stem##_bn_fin(M::Args a, const float2* __restrict__ part, int chans, int pstride, int pmul, int cnt, int mean_at,        \
                                      int rstd_at, float eps, float mom, float* __restrict__ run_mean, float* __restrict__ run_var) {            \
        tail_bn_fin_body<M>(a, part, chans, pstride, pmul, cnt, mean_at, rstd_at, eps, mom, run_mean, run_var);                                  \
    }                                                                                                                                             \
    template <bool TRAIN>                                                                                                                         \
    KGE_TAIL_KERNEL k_##stem##_fc(M::Args a, const float* __restrict__ conv, const float* __restrict__ m1f, int tiles, int f_per,                \
                                  float* __restrict__ upart) {                                                                                    \
        tail_fc_body<M, TRAIN>(a, conv, m1f, tiles, f_per, upart);                                                                                \
    }                                                                                                                                             \
    template <bool TRAIN>                                                                                                                         \
    KGE_TAIL_KERNEL k_##stem##_fc_finish(M::Args a, const float* __restrict__ upart, int splits, float eps, float mom,                           \
                                         float* __restrict__ run_mean, float* __restrict__ run_var, float* __restrict__ u,                       \
                                         float* __restrict__ x) {                                                                                 \
        tail_fc_finish_body<M, TRAIN>(a, upart, splits, eps, mom, run_mean, run_var, u, x);                                                       \
    }                                                                                                                                             \
    KGE_TAIL_KERNEL k_##stem##_bn2_bwd(M::Args a, const float* __restrict__ dx, const float* __restrict__ u, float* __restrict__ du,             \
                                       float* __restrict__ g_w2, float* __restrict__ g_b2, float* __restrict__ g_fcb) {                          \
        tail_bn2_bwd_body<M>(a, dx, u, du, g_w2, g_b2, g_fcb);                                                                                    \
    }                                                                                                                                             \
    KGE_TAIL_KERNEL k_##stem##_fc_gw(M::Args a, const float* __restrict__ conv, const float* __restrict__ m1f, const float* __restrict__ du,     \
                                     float* __restrict__ g_fc) {                                                                                  \
        tail_fc_gw_body<M>(a, conv, m1f, du, g_fc);                                                                                               \
    }                                                                                                                                             \
    KGE_TAIL_KERNEL k_##stem##_fc_da(M::Args a, const float* __restrict__ conv, const float* __restrict__ m1f, const float* __restrict__ du,     \
                                     int tiles, float* __restrict__ dy1) {                                                                        \
        tail_fc_da_body<M>(a, conv, m1f, du, tiles, dy1);                                                                                         \
    }                                                                                                                                             \
    KGE_TAIL_KERNEL k_##stem##_bn1_part(M::Args a, const float* __restrict__ conv, const float* __restrict__ dy1, float2* __restrict__ part) {   \
        tail_bn1_part_body<M>(a, conv, dy1, part);                                                                                                \
    }                                                                                                                                             \
    KGE_TAIL_KERNEL k_##stem##_bn1_bwd_fin(M::Args a, const float2* __restrict__ part, float2* __restrict__ sums, float* __restrict__ g_w1,      \
                                           float* __restrict__ g_b1) {                                                                            \
        tail_bn1_bwd_fin_body<M>(a, part, sums, g_w1, g_b1);                                                                                      \
    }                                                                                                                                             \
    KGE_TAIL_KERNEL k_##stem##_scatter(const int64_t* __restrict__ ids, int64_t n, int width, const float* __restrict__ src, int stride,         \
                                       float* __restrict__ dst) {                                                                                 \
        tail_scatter_body<SKIP0>(ids, n, width, src, stride, dst);                                                                                \
    }                                                                                                                                             \
    template <>                                                                                                                                   \
    struct TailKernels<M> {                                                                                                                       \
        static constexpr auto bn_fin = k_##stem##_bn_fin;                                                                                         \
        static constexpr auto fc_train = k_##stem##_fc<true>;                                                                                     \
        static constexpr auto fc_eval = k_##stem##_fc<false>;                                                                                     \
        static constexpr auto fc_finish_train = k_##stem##_fc_finish<true>;                                                                       \
        static constexpr auto fc_finish_eval = k_##stem##_fc_finish<false>;                                                                       \
        static constexpr auto bn2_bwd = k_##stem##_bn2_bwd;                                                                                       \
        static constexpr auto fc_gw = k_##stem##_fc_gw;                                                                                           \
        static constexpr auto fc_da = k_##stem##_fc_da;                                                                                           \
        static constexpr auto bn1_part = k_##stem##_bn1_part;                                                                                     \
        static constexpr auto bn1_bwd_fin = k_##stem##_bn1_bwd_fin;                                                                               \
        static constexpr auto scatter = k_##stem##_scatter;                                                                                       \
    };

// ------------------------------------------------------------------------------------------------------------------ host side
// momentum and eps of the three batch norms, the three dropout rates and the Philox offset of a descriptor
template <class D>
int tail_check_rates(const D* d, const char* who) {
    for (int i = 0; i < 3; ++i) {
        if (!(d->momentum[i] > 0.0f && d->momentum[i] <= 1.0f)) {
            set_error("%s: momentum %d must be in (0, 1] (got %g; the cumulative average is not built)", who, i, (double)d->momentum[i]);
            return -1;
        }
        if (!(d->eps[i] >= 0.0f)) { set_error("%s: eps %d must not be negative (got %g)", who, i, (double)d->eps[i]); return -1; }
    }
    const float p[3] = {d->input_dropout, d->feature_map_dropout, d->hidden_dropout};
    return drop_check(who, p, 3, d->offset);
}
// rows per direction of a call in training form
template <class D>
int tail_check_rows(const D* d, const char* who, int64_t n) {
    if (d->train && n == 1) {
        set_error("%s: batch norm in training form needs more than one row per direction (got n = 1)", who);
        return -1;
    }
    return 0;
}
// the part of a model's Args that the tail reads
template <class A, class D>
void tail_fill(A& a, const D* d, int64_t n, int dirs, int64_t row0, float* stats) {
    a.fcw = d->fc_w; a.fcb = d->fc_b; a.w1 = d->bn1_w; a.b1 = d->bn1_b; a.w2 = d->bn2_w; a.b2 = d->bn2_b;
    a.dirs = dirs; a.n = n; a.row0 = (uint32_t)row0;
    a.key = drop_key(d->seed, d->offset);
    const float p[3] = {d->input_dropout, d->feature_map_dropout, d->hidden_dropout};
    for (int i = 0; i < 3; ++i) {
        a.on[i] = d->train != 0 && p[i] > 0.0f;
        a.thr[i] = drop_thr(p[i]);
        a.scale[i] = drop_scale(p[i]);
    }
    a.stats = stats;
}

inline int tail_tiles(int64_t n) { return (int)((n + kTailRows - 1) / kTailRows); }
// f handled by one workgroup of the fc forward: enough workgroups to fill the device, a function of the shapes alone (the split order
// is the summation order); a multiple of 4
inline int tail_f_per(int K, int F, int64_t n, int dirs) {
    const int64_t base = (int64_t)dirs * tail_tiles(n) * ((K + 63) / 64);
    int64_t splits = (512 + base - 1) / base;
    if (splits > 64) splits = 64;
    if (splits < 1) splits = 1;
    int per = (int)((F + splits - 1) / splits);
    per = (per + 3) & ~3;
    return per < 4 ? 4 : per;
}
inline int tail_splits(int F, int per) { return (F + per - 1) / per; }
// upart [splits, N, K] of the fc forward
inline size_t tail_upart_bytes(int K, int F, int64_t n, int dirs) {
    return align256((size_t)tail_splits(F, tail_f_per(K, F, n, dirs)) * (size_t)n * dirs * K * sizeof(float));
}

// k_*_fc and k_*_fc_finish in the descriptor's form: conv (and m1f) -> u, x, bn2's statistics
template <class M>
int tail_fc_forward(const typename M::Desc* d, const typename M::Args& a, const float* conv, const float* m1f, float* upart, float* u, float* x,
                    hipStream_t st) {
    const int K = M::K(a), F = M::F(a);
    const int per = tail_f_per(K, F, a.n, a.dirs), splits = tail_splits(F, per), tiles = tail_tiles(a.n);
    const dim3 grid((unsigned)(a.dirs * tiles), (unsigned)((K + 63) / 64), (unsigned)splits);
    const unsigned col_blocks = (unsigned)((K + 3) / 4);
    if (d->train) {
        hipLaunchKernelGGL(TailKernels<M>::fc_train, grid, dim3(256), 0, st, a, conv, m1f, tiles, per, upart);
        hipLaunchKernelGGL(TailKernels<M>::fc_finish_train, dim3(col_blocks), dim3(256), 0, st, a, upart, splits, d->eps[2], d->momentum[2], d->bn2_mean,
                           d->bn2_var, u, x);
    } else {
        hipLaunchKernelGGL(TailKernels<M>::fc_eval, grid, dim3(256), 0, st, a, conv, m1f, tiles, per, upart);
        hipLaunchKernelGGL(TailKernels<M>::fc_finish_eval, dim3(col_blocks), dim3(256), 0, st, a, upart, splits, d->eps[2], d->momentum[2], d->bn2_mean,
                           d->bn2_var, u, x);
    }
    return check_launch("k_*_fc / k_*_fc_finish");
}

// the backward from dx down to dy1 and bn1's two sums (sums [dirs, C], g_bn1); part1 is float2 [N, C]; chan_groups is the y extent of
// k_*_bn1_part's grid.  The caller checks the last two launches with its next ones
template <class M>
int tail_backward(const typename M::Desc* d, const typename M::Args& a, const float* dx, const float* conv, const float* m1f, const float* u,
                  float* du, float* dy1, float2* part1, float2* sums, int chan_groups, hipStream_t st) {
    const int K = M::K(a), F = M::F(a), C = M::C(a), tiles = tail_tiles(a.n);
    const int64_t N = a.n * a.dirs;
    hipLaunchKernelGGL(TailKernels<M>::bn2_bwd, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, st, a, dx, u, du, d->g_bn2_w, d->g_bn2_b, d->g_fc_b);
    hipLaunchKernelGGL(TailKernels<M>::fc_gw, dim3((unsigned)((F + 63) / 64), (unsigned)((K + 127) / 128)), dim3(256), 0, st, a, conv, m1f, (const float*)du,
                       d->g_fc_w);
    hipLaunchKernelGGL(TailKernels<M>::fc_da, dim3((unsigned)(a.dirs * tiles), (unsigned)((F + 63) / 64)), dim3(256), 0, st, a, conv, m1f, (const float*)du,
                       tiles, dy1);
    if (int rc = check_launch("k_*_bn2_bwd / k_*_fc_gw / k_*_fc_da")) return rc;
    hipLaunchKernelGGL(TailKernels<M>::bn1_part, dim3((unsigned)N, (unsigned)chan_groups), dim3(256), 0, st, a, conv, (const float*)dy1, part1);
    hipLaunchKernelGGL(TailKernels<M>::bn1_bwd_fin, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, st, a, (const float2*)part1, sums, d->g_bn1_w, d->g_bn1_b);
    return 0;
}

template <class M>
void tail_scatter(const int64_t* ids, int64_t N, int width, const float* src, int stride, float* dst, hipStream_t st) {
    hipLaunchKernelGGL(TailKernels<M>::scatter, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, ids, N, width, src, stride, dst);
}

// ---- the entry points of include/kge_hip.h, one template each; `who` is the entry point's name
template <class M, size_t (*Bytes)(const typename M::Desc*, int64_t, int)>
size_t tail_bytes(const char* who, const typename M::Desc* d, int64_t n) {
    return M::check(d, who, false) || n < 0 ? 0 : Bytes(d, n > 0 ? n : 1, 1);
}

template <class M>
int tail_check_ids(const char* who, const typename M::Desc* d, const int64_t* e, const int64_t* r, int64_t n, hipStream_t s) {
    return check_er_ids(who, d->tot_entity, M::rel_rows(d), e, r, n, s);
}

template <class M>
int tail_body_forward(const char* who, const typename M::Desc* d, const int64_t* e, const int64_t* r, int64_t n, int32_t side, int64_t row0, float* x,
                      float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    if (M::check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!e || !r || !x || !saved)) || (side != 0 && side != 1) || row0 < 0 || row0 + n > 0xffffffffLL) {
        set_error("%s: bad arguments (%s)", who, M::kBadArgs);
        return -1;
    }
    if (tail_check_rows(d, who, n)) return -1;
    if (ws_check(who, workspace, workspace_bytes, M::fwd_bytes(d, n > 0 ? n : 1, 1))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = tail_check_ids<M>(who, d, e, r, n, s)) return rc;
    return M::forward(d, e, r, n, 1, side, row0, x, saved, workspace, s);
}

template <class M>
int tail_body_backward(const char* who, const typename M::Desc* d, const int64_t* e, const int64_t* r, int64_t n, int32_t side, int64_t row0,
                       const float* dx, const float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    if (M::check(d, who, true)) return -1;
    if (n < 0 || (n > 0 && (!e || !r || !dx || !saved)) || (side != 0 && side != 1) || row0 < 0 || row0 + n > 0xffffffffLL) {
        set_error("%s: bad arguments (%s)", who, M::kBadArgs);
        return -1;
    }
    if (!d->train) { set_error("%s: the eval form (train = 0) has no backward", who); return -1; }
    if (tail_check_rows(d, who, n)) return -1;
    if (ws_check(who, workspace, workspace_bytes, M::bwd_bytes(d, n > 0 ? n : 1, 1))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = tail_check_ids<M>(who, d, e, r, n, s)) return rc;
    return M::backward(d, e, r, n, 1, side, row0, dx, saved, workspace, s);
}

// fused step: ids [4B int64] | x [2B, K] | dx [2B, K] | saved | max(forward, backward, head)
struct TailStepPlan {
    size_t ids, x, dx, saved, rest, total;
};
template <class M>
TailStepPlan tail_step_plan(const typename M::Desc* d, int64_t B, int64_t n_hr, int64_t n_tr) {
    TailStepPlan p{};
    const size_t xb = align256((size_t)2 * B * M::dim(d) * sizeof(float));
    p.ids = 0;
    p.x = align256((size_t)4 * B * sizeof(int64_t));
    p.dx = p.x + xb;
    p.saved = p.dx + xb;
    p.rest = p.saved + align256(M::saved_floats(d, B, 2) * sizeof(float));
    size_t rest = M::fwd_bytes(d, B, 2);
    if (M::bwd_bytes(d, B, 2) > rest) rest = M::bwd_bytes(d, B, 2);
    const size_t h1 = kge_head_1n_bce_workspace_bytes(B, d->tot_entity, n_hr), h2 = kge_head_1n_bce_workspace_bytes(B, d->tot_entity, n_tr);
    if (h1 > rest) rest = h1;
    if (h2 > rest) rest = h2;
    p.total = p.rest + align256(rest);
    return p;
}

template <class M>
size_t tail_train_bce_bytes(const char* who, const typename M::Desc* d, int64_t batch, int64_t n_hr, int64_t n_tr) {
    if (M::check(d, who, false) || batch < 0 || n_hr < 0 || n_tr < 0) return 0;
    return tail_step_plan<M>(d, batch > 0 ? batch : 1, n_hr, n_tr).total;
}

template <class M>
int tail_train_bce(const char* who, const typename M::Desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t batch,
                   const int64_t* hr_off, const int32_t* hr_ids, int64_t n_hr, const int64_t* tr_off, const int32_t* tr_ids, int64_t n_tr,
                   float label_smoothing, void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    if (M::check(d, who, true)) return -1;
    if (batch < 0 || n_hr < 0 || n_tr < 0 || !loss || (batch > 0 && (!h || !r || !t || !hr_off || !tr_off)) || (n_hr > 0 && !hr_ids) ||
        (n_tr > 0 && !tr_ids) || 2 * batch > 0xffffffffLL) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    if (!d->train) { set_error("%s: the step is the training form (train = 0 has no backward)", who); return -1; }
    if (tail_check_rows(d, who, batch)) return -1;
    const TailStepPlan p = tail_step_plan<M>(d, batch > 0 ? batch : 1, n_hr, n_tr);
    if (ws_check(who, workspace, workspace_bytes, p.total)) return -1;
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t B = batch, n = 2 * B;
    const int k = M::dim(d);
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
    if (int rc = tail_check_ids<M>(who, d, e, rr, n, s)) return rc;
    // tail direction = forward(h, r, "tail") on rows 0 .. B-1, head direction = forward(t, r, "head") on rows B .. 2B-1, in the same launches
    if (int rc = M::forward(d, e, rr, B, 2, 0, 0, x, saved, rest, s)) return rc;
    if (int rc = kge_head_1n_bce(x, B, k, d->ent, d->tot_entity, M::bias(d), hr_off, hr_ids, n_hr, label_smoothing, rest, rest_bytes, loss, dx,
                                 d->g_ent, M::g_bias(d), stream)) return rc;
    if (int rc = kge_head_1n_bce(x + B * k, B, k, d->ent, d->tot_entity, M::bias(d), tr_off, tr_ids, n_tr, label_smoothing, rest, rest_bytes, loss,
                                 dx + B * k, d->g_ent, M::g_bias(d), stream)) return rc;
    return M::backward(d, e, rr, B, 2, 0, 0, dx, saved, rest, s);
}

// the rank pass's body (kge_projection.hip): the eval form on the rows [h; t] as two directions; ws = saved | the forward's workspace
template <class M>
int tail_eval_body(const void* desc, const int64_t* e, const int64_t* r, int64_t n, float* x, void* ws, size_t, hipStream_t s) {
    typename M::Desc ev = *(const typename M::Desc*)desc;
    ev.train = 0;
    const size_t saved = align256(M::saved_floats(&ev, n, 2) * sizeof(float));
    return M::forward(&ev, e, r, n, 2, 0, 0, x, (float*)ws, (char*)ws + saved, s);
}
template <class M>
ProjectionEval tail_eval(const typename M::Desc* d, int64_t n) {
    const int64_t rows = n > 0 ? n : 1;
    return ProjectionEval{M::dim(d), d->tot_entity, d->tot_relation, d->ent,
                          align256(M::saved_floats(d, rows, 2) * sizeof(float)) + M::fwd_bytes(d, rows, 2), tail_eval_body<M>, M::bias(d)};
}
template <class M>
size_t tail_eval_ranks_bytes(const char* who, const typename M::Desc* d, int64_t n) {
    return M::check(d, who, false) || n < 0 ? 0 : projection_eval_workspace_bytes(tail_eval<M>(d, n), n);
}
template <class M>
int tail_eval_ranks(const char* who, const typename M::Desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                    const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks, int32_t* ties,
                    void* stream) {
    if (M::check(d, who, false)) return -1;
    return projection_eval_ranks(who, tail_eval<M>(d, n), d, triples, n, tail_off, tail_ids, head_off, head_ids, workspace, workspace_bytes, ranks,
                                 ties, stream);
}

}  // namespace kge
