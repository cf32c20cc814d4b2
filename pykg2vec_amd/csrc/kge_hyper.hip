// kge_hyper.hip -- the body of HypER (models/projection.py:508-618) in front of the 1-N head of kge_head.hip.
// For a row with entity e and relation r, D = ent_hidden_size, Dr = rel_hidden_size, L = D - 8, F = 32 L:
//     y0   = bn0(ent[e]) * m0                                    one channel over the n D entity values; input dropout, site 0
//     filt = fc1_w rel[r] + fc1_b                                [32 channels][9 taps] PER ROW (k_hyper_filt, VALU); STORED in `saved`
//     c[ch, p] = sum_w y0[p + w] filt[ch, w]                     p in [0, L), no bias; VALU from the row in LDS (k_hyper_conv); STORED once
//     A    = bn1(c) * m1                                         NO relu; feature-map dropout, site 1: a whole channel of a row; never stored
//     u    = A fc_w^T + fc_b,  x = relu(bn2(u * m2))              the shared tail (kge_conv_tail.h); bn2 in BOTH forms (eval: running statistics)
// There is one relation table [R, Dr]; a direction selects nothing.  Training form: every batch norm normalises with the statistics
// of ITS DIRECTION's n rows and updates its running buffers, the tail direction first.  Statistics are fixed-order sums: per-row
// (mean, M2) partials over equal counts, combined over the rows in index order with the equal-count form of Chan's rule, as
// kge_conve.hip does.  Eval form (template parameter TRAIN = false): running statistics in bn0, bn1 and bn2, no draws, no writes.
//
// A call works on `dirs` directions of n rows each (body entry points: 1; fused step and rank pass: 2) in the SAME launches: row
// d n + b belongs to direction d.
//
// Backward (training form only), dx the gradient at x:
//     the shared tail     du, g_bn2, g_fc_b, g_fc, dy1 = (du x fc_w) * m1 and the two sums of bn1's backward with g_bn1
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
#include "kge_conv_tail.h"

namespace kge {

constexpr int kHyMaxK = KGE_HYPER_MAX_HIDDEN;   // both hidden sizes: eight relation rows (k_hyper_filt), the row and four channels of dc (k_hyper_conv_bwd) in LDS
constexpr int kHyCh = 32;           // output channels of the per-row filter
constexpr int kHyTaps = 9;          // filter width
constexpr int kHyQ = kHyCh * kHyTaps;   // fc1's outputs
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

// the tail's policy (kge_conv_tail.h)
struct HyTail {
    using Args = HyArgs;
    using Desc = kge_hyper_desc;
    static constexpr bool kClamp = false, kEvalBn2 = true;   // F = 32 L is a multiple of 16
    static constexpr const char* kBadArgs = "row0 + n below 2^32";
    __host__ __device__ static int K(const Args& a) { return a.D; }
    __host__ __device__ static int F(const Args& a) { return a.F; }
    __host__ __device__ static int C(const Args&) { return kHyCh; }
    __host__ __device__ static int E(const Args& a) { return a.L; }
    __host__ __device__ static int SS(const Args& a) { return 66 + 2 * a.D; }
    __host__ __device__ static int o1(const Args&) { return 2; }
    __host__ __device__ static int o2(const Args&) { return 66; }
    // A[row][f] = bn1(conv) * m1, formed from the stored conv output (no relu)
    template <bool TRAIN>
    __device__ __forceinline__ static float feature(const Args& a, const float* __restrict__ st, const float* __restrict__ conv, const float*, int64_t gr,
                                                    int f) {
        const int ch = f / a.L;
        float v = (conv[gr * a.F + f] - st[2 + ch]) * (st[34 + ch] * a.w1[ch]) + a.b1[ch];
        if constexpr (TRAIN) v *= tail_factor(a, 1, ch, gr);
        return v;
    }
    struct Bn1 {};
    __device__ __forceinline__ static Bn1 bn1_chan(const Args&, const float*, int) { return Bn1{}; }
    __device__ __forceinline__ static float dy1(const Args& a, const Bn1&, const float*, const float*, int64_t gr, int, int ch, float acc) {
        return acc * tail_factor(a, 1, ch, gr);
    }
    static int check(const Desc* d, const char* who, bool grads);
    static int dim(const Desc* d) { return d->ent_hidden_size; }
    static int64_t rel_rows(const Desc* d) { return d->tot_relation; }
    static const float* bias(const Desc* d) { return d->b; }
    static float* g_bias(const Desc* d) { return d->g_b; }
    static size_t saved_floats(const Desc* d, int64_t n, int dirs);
    static size_t fwd_bytes(const Desc* d, int64_t n, int dirs);
    static size_t bwd_bytes(const Desc* d, int64_t n, int dirs);
    static int forward(const Desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int side, int64_t row0, float* x, float* saved, void* ws,
                       hipStream_t st);
    static int backward(const Desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int side, int64_t row0, const float* dx,
                        const float* saved, void* ws, hipStream_t st);
};
KGE_CONV_TAIL_KERNELS(hyper, HyTail, true)

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
    const float* __restrict__ st = tail_stats<HyTail>(a, d);
    const float mean0 = st[0], g0 = st[1] * a.w0[0], b0 = a.b0[0];
    const float* __restrict__ src = a.ent + e[gr] * a.D;
    for (int p = threadIdx.x; p < a.D; p += 256) {
        float v = (src[p] - mean0) * g0 + b0;
        if constexpr (TRAIN) v *= tail_factor(a, 0, p, gr);
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

// ------------------------------------------------------------------------------------------------------------------ backward
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
    const float* __restrict__ st = tail_stats<HyTail>(a, d);
    const float mean0 = st[0], rstd0 = st[1], g0 = rstd0 * a.w0[0], b0 = a.b0[0];
    const float* __restrict__ src = a.ent + e[gr] * a.D;
    for (int p = threadIdx.x; p < a.D; p += 256) img[p] = ((src[p] - mean0) * g0 + b0) * tail_factor(a, 0, p, gr);
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
        const float v = accs[p] * tail_factor(a, 0, p, gr);
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
    const float* __restrict__ st = tail_stats<HyTail>(a, d);
    const float mean0 = st[0], rstd0 = st[1], gain = a.w0[0] * rstd0;
    const float2 T = t0[d];
    const float inv = 1.0f / ((float)a.n * (float)a.D);
    const float* __restrict__ src = a.ent + e[gr] * a.D;
    for (int p = lane; p < a.D; p += 64) {
        const float xh = (src[p] - mean0) * rstd0;
        dy0[gr * a.D + p] = gain * (dy0[gr * a.D + p] - T.x * inv - xh * (T.y * inv));
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

int HyTail::check(const kge_hyper_desc* d, const char* who, bool grads) {
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
    if (tail_check_rates(d, who)) return -1;
    if (grads) {
        const void* g[] = {d->g_b, d->g_ent, d->g_rel, d->g_bn0_w, d->g_bn0_b, d->g_bn1_w, d->g_bn1_b, d->g_bn2_w, d->g_bn2_b, d->g_fc_w, d->g_fc_b,
                           d->g_fc1_w, d->g_fc1_b};
        for (const void* q : g)
            if (!q) { set_error("%s: null gradient buffers (all 13 are required)", who); return -1; }
    }
    return 0;
}

static HyArgs hy_args(const kge_hyper_desc* d, int64_t n, int dirs, int64_t row0, float* stats) {
    const HyShape s = hy_shape(d);
    HyArgs a{};
    tail_fill(a, d, n, dirs, row0, stats);
    a.ent = d->ent; a.rel = d->rel; a.w0 = d->bn0_w; a.b0 = d->bn0_b; a.f1w = d->fc1_w; a.f1b = d->fc1_b;
    a.D = s.D; a.Dr = s.Dr; a.L = s.L; a.F = s.F;
    return a;
}

// saved (floats): conv [N, F] | u [N, D] | filt [N, 288] | stats [dirs][66 + 2D]
size_t HyTail::saved_floats(const kge_hyper_desc* d, int64_t n, int dirs) {
    const HyShape s = hy_shape(d);
    return (size_t)dirs * ((size_t)n * ((size_t)s.F + s.D + kHyQ) + 66 + 2 * (size_t)s.D);
}
// forward: row partials float2 [N, 32] | upart [splits, N, D]
size_t HyTail::fwd_bytes(const kge_hyper_desc* d, int64_t n, int dirs) {
    const HyShape s = hy_shape(d);
    const size_t N = (size_t)n * dirs;
    return align256(N * kHyCh * sizeof(float2)) + tail_upart_bytes(s.D, s.F, n, dirs);
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
size_t HyTail::bwd_bytes(const kge_hyper_desc* d, int64_t n, int dirs) { return hy_bwd_plan(d, n, dirs).total; }

int HyTail::forward(const kge_hyper_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int, int64_t row0, float* x, float* saved,
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
        hipLaunchKernelGGL(k_hyper_bn_fin, dim3(1), dim3(256), 0, st, a, part, 1, 1, 1, s.D, 0, 1, d->eps[0], d->momentum[0], d->bn0_mean, d->bn0_var);
        hipLaunchKernelGGL((k_hyper_conv<true>), dim3((unsigned)N), dim3(256), 0, st, a, e, filt, conv, part);
        if (int rc = check_launch("k_hyper_filt / k_hyper_row_stats / k_hyper_bn_fin / k_hyper_conv")) return rc;
        hipLaunchKernelGGL(k_hyper_bn_fin, dim3(kHyCh / 4), dim3(256), 0, st, a, part, kHyCh, kHyCh, 1, s.L, 2, 34, d->eps[1], d->momentum[1],
                           d->bn1_mean, d->bn1_var);
    } else {
        hipLaunchKernelGGL(k_hyper_stats_eval, dim3(1), dim3(256), 0, st, a, d->eps[0], d->eps[1], d->eps[2], d->bn0_mean, d->bn0_var, d->bn1_mean,
                           d->bn1_var, d->bn2_mean, d->bn2_var);
        hipLaunchKernelGGL((k_hyper_conv<false>), dim3((unsigned)N), dim3(256), 0, st, a, e, filt, conv, part);
    }
    return tail_fc_forward<HyTail>(d, a, conv, nullptr, upart, u, x, st);
}

int HyTail::backward(const kge_hyper_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int, int64_t row0, const float* dx,
                     const float* saved, void* ws, hipStream_t st) {
    const HyShape s = hy_shape(d);
    const int64_t N = n * dirs;
    const float *conv = saved, *u = conv + N * s.F, *filt = u + N * s.D;
    const HyArgs a = hy_args(d, n, dirs, row0, const_cast<float*>(filt + N * kHyQ));
    const HyBwdPlan p = hy_bwd_plan(d, n, dirs);
    char* w = (char*)ws;
    float *du = (float*)(w + p.du), *dy1 = (float*)(w + p.dy1), *dfilt = (float*)(w + p.dfilt), *dy0 = (float*)(w + p.dy0), *drel = (float*)(w + p.drel);
    float2 *part1 = (float2*)(w + p.part1), *sums = (float2*)(w + p.sums), *pt0 = (float2*)(w + p.pt0), *t0 = (float2*)(w + p.t0);
    const unsigned row_blocks = (unsigned)((N + 3) / 4);
    const unsigned row2_blocks = (unsigned)((N + kHyDR - 1) / kHyDR);
    if (int rc = tail_backward<HyTail>(d, a, dx, conv, nullptr, u, du, dy1, part1, sums, 1, st)) return rc;
    hipLaunchKernelGGL(k_hyper_conv_bwd, dim3((unsigned)N), dim3(256), 0, st, a, e, filt, conv, dy1, sums, dfilt, dy0, pt0);
    if (int rc = check_launch("k_hyper_bn1_part / k_hyper_bn1_bwd_fin / k_hyper_conv_bwd")) return rc;
    hipLaunchKernelGGL(k_hyper_small_fin, dim3((kHyQ + 1 + 3) / 4), dim3(256), 0, st, a, dfilt, pt0, t0, d->g_fc1_b, d->g_bn0_w, d->g_bn0_b);
    hipLaunchKernelGGL(k_hyper_fc1_gw, dim3((unsigned)((kHyQ * s.Dr + 255) / 256)), dim3(256), 0, st, a, r, dfilt, d->g_fc1_w);
    hipLaunchKernelGGL(k_hyper_drel, dim3(row2_blocks), dim3(256), 0, st, a, dfilt, N, drel);
    hipLaunchKernelGGL(k_hyper_dent, dim3(row_blocks), dim3(256), 0, st, a, e, t0, dy0);
    if (int rc = check_launch("k_hyper_small_fin / k_hyper_fc1_gw / k_hyper_drel / k_hyper_dent")) return rc;
    tail_scatter<HyTail>(e, N, s.D, dy0, s.D, d->g_ent, st);   // (id 0 is skipped on both tables: padding_idx = 0)
    tail_scatter<HyTail>(r, N, s.Dr, drel, s.Dr, d->g_rel, st);
    return check_launch("k_hyper_scatter");
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_hyper_saved_floats(const kge_hyper_desc* d, int64_t n) {
    return tail_bytes<HyTail, HyTail::saved_floats>("kge_hyper_saved_floats", d, n);
}

size_t kge_hyper_body_forward_workspace_bytes(const kge_hyper_desc* d, int64_t n) {
    return tail_bytes<HyTail, HyTail::fwd_bytes>("kge_hyper_body_forward_workspace_bytes", d, n);
}

int kge_hyper_body_forward(const kge_hyper_desc* d, const int64_t* e, const int64_t* r, int64_t n, int64_t row0, float* x, float* saved,
                           void* workspace, size_t workspace_bytes, void* stream) {
    return tail_body_forward<HyTail>("kge_hyper_body_forward", d, e, r, n, 0, row0, x, saved, workspace, workspace_bytes, stream);
}

size_t kge_hyper_body_backward_workspace_bytes(const kge_hyper_desc* d, int64_t n) {
    return tail_bytes<HyTail, HyTail::bwd_bytes>("kge_hyper_body_backward_workspace_bytes", d, n);
}

int kge_hyper_body_backward(const kge_hyper_desc* d, const int64_t* e, const int64_t* r, int64_t n, int64_t row0, const float* dx,
                            const float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    return tail_body_backward<HyTail>("kge_hyper_body_backward", d, e, r, n, 0, row0, dx, saved, workspace, workspace_bytes, stream);
}

size_t kge_hyper_train_bce_workspace_bytes(const kge_hyper_desc* d, int64_t batch, int64_t n_hr, int64_t n_tr) {
    return tail_train_bce_bytes<HyTail>("kge_hyper_train_bce_workspace_bytes", d, batch, n_hr, n_tr);
}

int kge_hyper_train_bce(const kge_hyper_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t batch, const int64_t* hr_off,
                        const int32_t* hr_ids, int64_t n_hr, const int64_t* tr_off, const int32_t* tr_ids, int64_t n_tr, float label_smoothing,
                        void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    return tail_train_bce<HyTail>("kge_hyper_train_bce", d, h, r, t, batch, hr_off, hr_ids, n_hr, tr_off, tr_ids, n_tr, label_smoothing, workspace,
                                  workspace_bytes, loss, stream);
}

size_t kge_hyper_eval_ranks_workspace_bytes(const kge_hyper_desc* d, int64_t n) {
    return tail_eval_ranks_bytes<HyTail>("kge_hyper_eval_ranks_workspace_bytes", d, n);
}

int kge_hyper_eval_ranks(const kge_hyper_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                         const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks, int32_t* ties,
                         void* stream) {
    return tail_eval_ranks<HyTail>("kge_hyper_eval_ranks", d, triples, n, tail_off, tail_ids, head_off, head_ids, workspace, workspace_bytes, ranks,
                                   ties, stream);
}

}  // extern "C"
