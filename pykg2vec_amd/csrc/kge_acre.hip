// kge_acre.hip -- the body of AcrE (models/projection.py:621-746) in front of the 1-N head of kge_head.hip.
// K = hidden_size = 200, the image is always H x W = 20 x 20 (HW = 400 = 2K), C = in_channels, a1 / a2 / a3 the three dilations,
// F = 400 C.  For a row with entity e and relation r, in the SERIAL way (way = 0; the PARALLEL way, way = 1, shares everything before
// z1 and after c and is described at its kernels, k_acrp_*, below):
//     img = [ent[e] | rel[r]] viewed [20, 20]                  ONE relation table [2R, K]; a direction selects nothing
//     y0  = bn0(img) * m0                                      input dropout, site 0; res = y0
//     z1  = conv1(y0)   1 -> C, 3 x 3, dilation a1, zero padding a1      VALU from y0 in LDS (k_acre_conv1), STORED
//     z2  = conv2(z1)   C -> C, dilation a2                    an implicit GEMM on v_mfma_f32_16x16x4_f32 (k_acre_cc): per row
//     z3  = conv3(z2)   C -> C, dilation a3                    M = C output channels, N = 400 positions, K = 9 C; the input layer is
//                                                              held in LDS, a tap that falls into the padding is a zero operand and
//                                                              C is padded to the tile by zero operands (nothing padded in memory)
//     c   = z3 + res (res broadcast over the channels)         added in k_acre_cc's epilogue; z2 and c STORED
//     A   = relu(bn1(c)) * m1                                  feature-map dropout, site 1: a whole channel of a row; never stored
//     u   = A fc_w^T + fc_b,  x = relu(bn2(u * m2))             the shared tail (kge_conv_tail.h); bn2 in BOTH forms
// Every convolution has a bias iff acre_bias.  There is no nonlinearity between the three convolutions.  Batch norm, the two forms,
// the statistics as fixed-order (mean, M2) sums and `dirs` are those of kge_interacte.hip.
//
// Backward (training form only), dx the gradient at x:
//     the shared tail   du, g_bn2, g_fc_b, g_fc, dy1 = (du x fc_w) * m1 [bn1 > 0] and the two sums of bn1's backward with g_bn1
//     k_acre_bn1_dc     dc = d loss / d c through bn1, in place of dy1; dz3 = dc and d res = sum over the channels of dc, ascending
//     k_acre_cc_gw      per row: gwp[row][o, i, t] = sum_pos dz[o, pos] in[i, pos + tap t] on the matrix cores (M = o, N = i, the 400
//                       positions are the contraction; both layers in LDS) and the bias partial gbp[row][o] = sum_pos dz[o, pos]
//     k_acre_cc<true>   dz_in = the same implicit GEMM with the flipped, transposed filter
//     k_acre_c1_bwd     per row: conv1's filter and bias partials (VALU), dy0 = (conv1^T dz1 + d res) * m0, bn0's two row sums
//     k_acre_rowsum     g += the per-row partials: 16 row classes (row mod 16) each in row order, then the 16 sums as a fixed tree
//     k_acre_bn0_fin / k_acre_dcomb / k_acre_scatter    bn0's backward, d ent | d rel rows, the ordered scatter (every id, 0 included)
// z1 and z2 are SAVED by the forward, not recomputed: they pass through global memory between the launches anyway.
// The parallel way replaces the chain and the residual by z_i = conv_i(y0), i = 1 .. 3 (k_acre_conv1 three times) and the gate
//     c[ch] = [y0 | z_1[ch] | z_2[ch] | z_3[ch]] gate_w^T + gate_b        a GEMM over the (row, channel) pairs (k_acrp_gate)
// and its backward by k_acrp_chsum / k_acrp_gate_gw / k_acrp_gw_fin (g_gate_w, g_gate_b), k_acrp_gate (dres, dz_i) and
// k_acrp_conv_bwd (the three convolutions of y0 at once).  It SAVES c, z_1, z_2, z_3.
// No kernel of this file uses atomics.
//
// The dropout draw is the shared one (kge_projection.h spells the Philox counters out), with
//     site 0: elem = pixel in [0, 400), entity half first;   site 1: elem = channel in [0, C);   site 2: elem = j in [0, K)
//     row = row0 + position in the call's row list.  The fused step numbers the h rows 0 .. B-1 and the t rows B .. 2B-1.
#include "kge_conv_tail.h"

namespace kge {

constexpr int kAcK = 200;           // hidden_size
constexpr int kAcW = 20;            // image width and height
constexpr int kAcHW = 400;
constexpr int kAcMaxC = KGE_ACRE_MAX_CHANNELS;
constexpr int kAcLS = 404;          // LDS stride of a channel's 400 values: 16 channels at one position fall on 16 distinct banks
constexpr int kAcPT = 7;            // position tiles (of 16) per wave of k_acre_cc: 25 tiles over 4 waves
static_assert(kAcMaxC % 16 == 0 && 4 * kAcPT >= kAcHW / 16 && kAcHW % 16 == 0, "tiles");

struct AcArgs {
    const float *ent, *rel, *w0, *b0, *w1, *b1, *w2, *b2, *fcw, *fcb;
    const float *cw[3], *cb[3];     // conv weights [C, 1 or C, 3, 3] and biases [C] (NULL without acre_bias)
    int dil[3];
    int K, HW, C, F;
    int dirs;
    int64_t n;                      // rows per direction
    uint32_t row0;
    int on[3];                      // site draws (training form and p > 0)
    DropKey key;
    uint32_t thr[3];
    float scale[3];
    float* stats;                   // [dirs][SS]: mean0, rstd0, mean1[C], rstd1[C], mean2[K], rstd2[K]
    int SS, o1, o2;                 // SS = 2 + 2C + 2K, o1 = 2, o2 = 2 + 2C
};

// the tail's policy (kge_conv_tail.h), both ways
struct AcTail : TailReluM1f<AcArgs> {
    using Desc = kge_acre_desc;
    static constexpr const char* kBadArgs = "row0 + n below 2^32";
    static int check(const Desc* d, const char* who, bool grads);
    static int dim(const Desc*) { return kAcK; }
    static int64_t rel_rows(const Desc* d) { return 2 * d->tot_relation; }   // (the relation table has 2 tot_relation rows, every one an ordinary row)
    static const float* bias(const Desc* d) { return d->bias; }
    static float* g_bias(const Desc* d) { return d->g_bias; }
    static size_t saved_floats(const Desc* d, int64_t n, int dirs);
    static size_t fwd_bytes(const Desc* d, int64_t n, int dirs);
    static size_t bwd_bytes(const Desc* d, int64_t n, int dirs);
    static int forward(const Desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int side, int64_t row0, float* x, float* saved, void* ws,
                       hipStream_t st);
    static int backward(const Desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int side, int64_t row0, const float* dx,
                        const float* saved, void* ws, hipStream_t st);
};
KGE_CONV_TAIL_KERNELS(acre, AcTail, false)

__device__ __forceinline__ float ac_comb(const AcArgs& a, const float* __restrict__ er, const float* __restrict__ rr, int c) {
    return c < a.K ? er[c] : rr[c - a.K];
}
// position of tap t (0 .. 8) of a 3 x 3 filter with dilation d around pos, or -1 in the zero padding
__device__ __forceinline__ int ac_tap(int pos, int t, int d) {
    const int y = pos / kAcW + (t / 3 - 1) * d, x = pos % kAcW + (t % 3 - 1) * d;
    return (y >= 0 && y < kAcW && x >= 0 && x < kAcW) ? y * kAcW + x : -1;
}

__device__ __forceinline__ double ac_wave_sum_xor(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per row: (mean, M2) of the row's 400 values [ent[e] | rel[r]], summed in double: the mean of zero-centred embeddings
// nearly cancels, and bn0's running mean is compared on its own size
__global__ void __launch_bounds__(256) k_acre_row_stats(AcArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                        double2* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t gr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gr >= a.n * a.dirs) return;
    const float* __restrict__ er = a.ent + e[gr] * a.K;
    const float* __restrict__ rr = a.rel + r[gr] * a.K;
    double s = 0.0;
    for (int c = lane; c < a.HW; c += 64) s += (double)ac_comb(a, er, rr, c);
    const double mean = ac_wave_sum_xor(s) / (double)a.HW;
    double m2 = 0.0;
    for (int c = lane; c < a.HW; c += 64) { const double v = (double)ac_comb(a, er, rr, c) - mean; m2 += v * v; }
    m2 = ac_wave_sum_xor(m2);
    if (lane == 0) part[gr] = make_double2(mean, m2);
}

// one wave: bn0's statistics of every direction from the per-row partials (each over 400 values), in double, the tail direction
// first; mean / rstd -> stats, running buffers updated (momentum, unbiased variance)
__global__ void __launch_bounds__(64) k_acre_bn0_stats(AcArgs a, const double2* __restrict__ part, float eps, float mom,
                                                       float* __restrict__ run_mean, float* __restrict__ run_var) {
    const int lane = threadIdx.x;
    for (int d = 0; d < a.dirs; ++d) {
        const double2* __restrict__ p = part + (size_t)d * a.n;
        double s = 0.0;
        for (int64_t b = lane; b < a.n; b += 64) s += p[b].x;
        const double mean = ac_wave_sum_xor(s) / (double)a.n;
        double m2 = 0.0;
        for (int64_t b = lane; b < a.n; b += 64) { const double2 v = p[b]; const double dv = v.x - mean; m2 += v.y + (double)a.HW * (dv * dv); }
        m2 = ac_wave_sum_xor(m2);
        const double tot = (double)a.n * (double)a.HW;
        if (lane == 0) {
            float* st = a.stats + (size_t)d * a.SS;
            const float meanf = (float)mean;
            st[0] = meanf;
            st[1] = 1.0f / sqrtf((float)(m2 / tot) + eps);
            run_mean[0] = (1.0f - mom) * run_mean[0] + mom * meanf;
            run_var[0] = (1.0f - mom) * run_var[0] + mom * (float)(m2 / (tot - 1.0));
        }
    }
}

// eval form: bn0, bn1 and bn2 normalise with the running buffers
__global__ void __launch_bounds__(256) k_acre_stats_eval(AcArgs a, float eps0, float eps1, float eps2, const float* __restrict__ rm0,
                                                         const float* __restrict__ rv0, const float* __restrict__ rm1,
                                                         const float* __restrict__ rv1, const float* __restrict__ rm2,
                                                         const float* __restrict__ rv2) {
    const int t0 = (int)blockIdx.x * 256 + threadIdx.x;
    for (int d = 0; d < a.dirs; ++d) {
        float* st = a.stats + (size_t)d * a.SS;
        for (int t = t0; t < 1 + a.C + a.K; t += (int)gridDim.x * 256) {
            if (t < 1) { st[0] = rm0[0]; st[1] = 1.0f / sqrtf(rv0[0] + eps0); }
            else if (t < 1 + a.C) { const int c = t - 1; st[a.o1 + c] = rm1[c]; st[a.o1 + a.C + c] = 1.0f / sqrtf(rv1[c] + eps1); }
            else { const int j = t - 1 - a.C; st[a.o2 + j] = rm2[j]; st[a.o2 + a.K + j] = 1.0f / sqrtf(rv2[j] + eps2); }
        }
    }
}

// y0 = bn0(img) * m0 of row gr as 400 floats in LDS.  All 256 threads; ends with a barrier
__device__ __forceinline__ void ac_load_y0(const AcArgs& a, const float* __restrict__ st, const int64_t* __restrict__ e,
                                           const int64_t* __restrict__ r, int64_t gr, float* __restrict__ y0s) {
    const float mean0 = st[0], g0 = st[1] * a.w0[0], b0 = a.b0[0];
    const float* __restrict__ er = a.ent + e[gr] * a.K;
    const float* __restrict__ rr = a.rel + r[gr] * a.K;
    for (int pix = threadIdx.x; pix < kAcHW; pix += 256)
        y0s[pix] = ((ac_comb(a, er, rr, pix) - mean0) * g0 + b0) * tail_factor(a, 0, pix, gr);
    __syncthreads();
}
// the C channels of row gr of a stored layer [N, F] into LDS with channel stride kAcLS.  All 256 threads; ends with a barrier
__device__ __forceinline__ void ac_load_layer(const AcArgs& a, const float* __restrict__ src, int64_t gr, float* __restrict__ ls) {
    const float* __restrict__ s = src + gr * a.F;
    for (int idx = threadIdx.x; idx < a.F; idx += 256) { const int ch = idx / kAcHW; ls[ch * kAcLS + (idx - ch * kAcHW)] = s[idx]; }
    __syncthreads();
}

// one workgroup per row, one wave per output channel: out[o, pos] = b[o] + sum_t w[o, t] y0[pos + tap t], layer L's filter and dilation
__global__ void __launch_bounds__(256) k_acre_conv1(AcArgs a, int L, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                    float* __restrict__ out) {
    __shared__ float y0s[kAcHW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    ac_load_y0(a, tail_stats<AcTail>(a, (int)(gr / a.n)), e, r, gr, y0s);
    const int d = a.dil[L];
    for (int o = wave; o < a.C; o += 4) {
        float w[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) w[t] = a.cw[L][o * 9 + t];
        const float bias = a.cb[L] ? a.cb[L][o] : 0.0f;
        float* __restrict__ dst = out + gr * a.F + (int64_t)o * kAcHW;
        for (int pos = lane; pos < kAcHW; pos += 64) {
            float v = bias;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int sp = ac_tap(pos, t, d);
                v += w[t] * (sp >= 0 ? y0s[sp] : 0.0f);
            }
            dst[pos] = v;
        }
    }
}

// one workgroup per row: the C -> C dilated convolution of layer L as an implicit GEMM.  The input layer sits in LDS; wave w owns the
// position tiles w, w + 4, ... (16 positions each, at most kAcPT) for every block of 16 output channels.  Operands of one
// v_mfma_f32_16x16x4_f32: A[m = channel l][k = input channel g] = the filter value of tap t, B[k = g][n = position l] = the input at the
// tap's place or 0 in the padding; the contraction runs over the taps and the input channels in blocks of 4.
// BWD = false: out[o, pos] = b[o] + sum_{i, t} w[o, i, t] in[i, pos + tap t]  (+ y0[pos] when addres: the residual)
// BWD = true:  out[i, pos] = sum_{o, t} w[o, i, t] in[o, pos - tap t]: the filter transposed and flipped (tap 8 - t), no bias
template <bool BWD>
__global__ void __launch_bounds__(256) k_acre_cc(AcArgs a, int L, int addres, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                 const float* __restrict__ in, float* __restrict__ out) {
    __shared__ float ls[kAcMaxC * kAcLS];
    __shared__ float y0s[kAcHW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int64_t gr = blockIdx.x;
    if (addres) ac_load_y0(a, tail_stats<AcTail>(a, (int)(gr / a.n)), e, r, gr, y0s);
    ac_load_layer(a, in, gr, ls);
    const int d = a.dil[L], C = a.C;
    const float* __restrict__ w = a.cw[L];
    for (int ot = 0; ot < (C + 15) / 16; ++ot) {
        const int ol = 16 * ot + l;          // the A operand's channel
        const bool olok = ol < C;
        f32x4v acc[kAcPT];
#pragma unroll
        for (int j = 0; j < kAcPT; ++j) acc[j] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
        for (int t = 0; t < 9; ++t) {
            int sp[kAcPT];
#pragma unroll
            for (int j = 0; j < kAcPT; ++j) {
                const int pt = wave + 4 * j;
                sp[j] = pt < kAcHW / 16 ? ac_tap(16 * pt + l, t, d) : -1;
            }
            for (int i0 = 0; i0 < C; i0 += 4) {
                const int i = i0 + g;
                const bool iok = i < C;
                const int ic = iok ? i : C - 1;
                float av = 0.0f;
                if (olok && iok) av = BWD ? w[(i * C + ol) * 9 + (8 - t)] : w[(ol * C + i) * 9 + t];
                const float* __restrict__ lrow = ls + ic * kAcLS;
#pragma unroll
                for (int j = 0; j < kAcPT; ++j) {
                    if (wave + 4 * j >= kAcHW / 16) continue;   // (wave-uniform)
                    const float bv = (iok && sp[j] >= 0) ? lrow[sp[j] >= 0 ? sp[j] : 0] : 0.0f;
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kAcPT; ++j) {
            const int pt = wave + 4 * j;
            if (pt >= kAcHW / 16) continue;
            const int pos = 16 * pt + l;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = 16 * ot + 4 * g + q;
                if (o >= C) continue;
                float v = acc[j][q];
                if constexpr (!BWD) {
                    if (a.cb[L]) v += a.cb[L][o];
                    if (addres) v += y0s[pos];
                }
                out[gr * a.F + (int64_t)o * kAcHW + pos] = v;
            }
        }
    }
}

// one wave per (row, channel): the channel's (mean, M2) over the row's 400 values of c -> part[row][C], and its feature-map factor
__global__ void __launch_bounds__(256) k_acre_c_stats(AcArgs a, const float* __restrict__ c, float2* __restrict__ part, float* __restrict__ m1f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    for (int ch = (int)blockIdx.y * 4 + wave; ch < a.C; ch += 4 * (int)gridDim.y) {
        const float* __restrict__ src = c + gr * a.F + (int64_t)ch * kAcHW;
        float s = 0.0f;
        for (int pos = lane; pos < kAcHW; pos += 64) s += src[pos];
        const float mean = wave_sum_xor(s) / (float)kAcHW;
        float m2 = 0.0f;
        for (int pos = lane; pos < kAcHW; pos += 64) { const float v = src[pos] - mean; m2 += v * v; }
        m2 = wave_sum_xor(m2);
        if (lane == 0) {
            part[gr * a.C + ch] = make_float2(mean, m2);
            m1f[gr * a.C + ch] = tail_factor(a, 1, ch, gr);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// one wave per (row, channel): dc = w1 rstd1 (dy1 - S1 / N1 - xh1 S2 / N1), written over dy1 IN PLACE (a lane reads and writes its own
// positions)
__global__ void __launch_bounds__(256) k_acre_bn1_dc(AcArgs a, const float* __restrict__ conv, float* __restrict__ dy1,
                                                     const float2* __restrict__ sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    const int d = (int)(gr / a.n);
    const float* __restrict__ st = tail_stats<AcTail>(a, d);
    const float invN1 = 1.0f / ((float)a.n * (float)a.HW);
    for (int ch = (int)blockIdx.y * 4 + wave; ch < a.C; ch += 4 * (int)gridDim.y) {
        const float mean = st[a.o1 + ch], rstd = st[a.o1 + a.C + ch], gain = a.w1[ch] * rstd;
        const float2 S = sums[d * a.C + ch];
        const int64_t base = gr * a.F + (int64_t)ch * a.HW;
        for (int pos = lane; pos < a.HW; pos += 64) {
            const float xh = (conv[base + pos] - mean) * rstd;
            dy1[base + pos] = gain * (dy1[base + pos] - S.x * invN1 - xh * (S.y * invN1));
        }
    }
}

// one workgroup per row: the filter partials of a C -> C layer, gwp[row][(o C + i) 9 + t] = sum_pos dz[o, pos] in[i, pos + tap t], and
// gbp[row][o] = sum_pos dz[o, pos].  Both layers sit in LDS (103 424 bytes: one workgroup per compute unit).  A wave takes the
// (tap, 16 o, 16 i) tiles wave, wave + 4, ...; operands of one v_mfma_f32_16x16x4_f32: A[m = o l][k = position g] = dz,
// B[k = g][n = i l] = the input at the tap's place or 0; the 400 positions are the contraction, in blocks of 4, ascending
__global__ void __launch_bounds__(256) k_acre_cc_gw(AcArgs a, int L, const float* __restrict__ dz, const float* __restrict__ in,
                                                    float* __restrict__ gwp, float* __restrict__ gbp) {
    __shared__ float dzs[kAcMaxC * kAcLS];
    __shared__ float ins[kAcMaxC * kAcLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int64_t gr = blockIdx.x;
    const int d = a.dil[L], C = a.C, CT = (C + 15) / 16;
    ac_load_layer(a, dz, gr, dzs);
    ac_load_layer(a, in, gr, ins);
    for (int task = wave; task < 9 * CT * CT; task += 4) {
        const int t = task / (CT * CT), ot = (task / CT) % CT, it = task % CT;
        const int ol = 16 * ot + l, il = 16 * it + l;
        const bool ook = ol < C, iok = il < C;
        const float* __restrict__ drow = dzs + (ook ? ol : 0) * kAcLS;
        const float* __restrict__ irow = ins + (iok ? il : 0) * kAcLS;
        f32x4v acc = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
        for (int p0 = 0; p0 < kAcHW; p0 += 4) {
            const int pos = p0 + g, sp = ac_tap(pos, t, d);
            const float av = ook ? drow[pos] : 0.0f;
            const float bv = (iok && sp >= 0) ? irow[sp >= 0 ? sp : 0] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
        if (iok)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = 16 * ot + 4 * g + q;
                if (o < C) gwp[gr * (int64_t)(9 * C * C) + (o * C + il) * 9 + t] = acc[q];
            }
    }
    if (gbp)
        for (int o = wave; o < C; o += 4) {
            float s = 0.0f;
            for (int pos = lane; pos < kAcHW; pos += 64) s += dzs[o * kAcLS + pos];
            s = wave_sum_xor(s);
            if (lane == 0) gbp[gr * C + o] = s;
        }
}

// one workgroup per row, the 1 -> C layer L whose input is y0.  One wave per channel o: gwp[row][o 9 + t] = sum_pos dz[o, pos]
// y0[pos + tap t] and gbp[row][o] = sum_pos dz[o, pos].  Then a thread per pixel: the transposed convolution sum_{o, t} w[o, t]
// dz[o, pix - tap t] (o ascending) plus, with dc, the residual's gradient sum_ch dc[ch, pix] (ch ascending);
// dy0 = that * m0 -> dimg[row][400]; (sum dy0, sum dy0 xh0) -> pt0[row]
__global__ void __launch_bounds__(256) k_acre_c1_bwd(AcArgs a, int L, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                     const float* __restrict__ dz, const float* __restrict__ dc, float* __restrict__ gwp,
                                                     float* __restrict__ gbp, float* __restrict__ dimg, float2* __restrict__ pt0) {
    __shared__ float dzs[kAcMaxC * kAcLS];
    __shared__ float y0s[kAcHW];
    __shared__ float wl[kAcMaxC * 9];
    __shared__ float red[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x;
    const float* __restrict__ st = tail_stats<AcTail>(a, (int)(gr / a.n));
    const int d = a.dil[L], C = a.C;
    for (int i = threadIdx.x; i < 9 * C; i += 256) wl[i] = a.cw[L][i];
    ac_load_y0(a, st, e, r, gr, y0s);
    ac_load_layer(a, dz, gr, dzs);
    for (int o = wave; o < C; o += 4) {
        const float* __restrict__ drow = dzs + o * kAcLS;
        float sb = 0.0f;
        for (int pos = lane; pos < kAcHW; pos += 64) sb += drow[pos];
        sb = wave_sum_xor(sb);
        if (lane == 0 && gbp) gbp[gr * C + o] = sb;
        for (int t = 0; t < 9; ++t) {
            float s = 0.0f;
            for (int pos = lane; pos < kAcHW; pos += 64) {
                const int sp = ac_tap(pos, t, d);
                s += drow[pos] * (sp >= 0 ? y0s[sp] : 0.0f);
            }
            s = wave_sum_xor(s);
            if (lane == 0) gwp[gr * (int64_t)(9 * C) + o * 9 + t] = s;
        }
    }
    const float mean0 = st[0], rstd0 = st[1];
    const float* __restrict__ er = a.ent + e[gr] * a.K;
    const float* __restrict__ rr = a.rel + r[gr] * a.K;
    float t1 = 0.0f, t2 = 0.0f;
    for (int pix = threadIdx.x; pix < kAcHW; pix += 256) {
        int sp[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) sp[t] = ac_tap(pix, 8 - t, d);   // pix - tap t
        float v = 0.0f;
        for (int o = 0; o < C; ++o) {
            float s = 0.0f;
#pragma unroll
            for (int t = 0; t < 9; ++t) s += wl[o * 9 + t] * (sp[t] >= 0 ? dzs[o * kAcLS + (sp[t] >= 0 ? sp[t] : 0)] : 0.0f);
            v += s;
        }
        if (dc) {
            float rs = 0.0f;
            for (int ch = 0; ch < C; ++ch) rs += dc[gr * a.F + (int64_t)ch * kAcHW + pix];
            v += rs;
        }
        v *= tail_factor(a, 0, pix, gr);
        dimg[gr * kAcHW + pix] = v;
        t1 += v;
        t2 += v * ((ac_comb(a, er, rr, pix) - mean0) * rstd0);
    }
    t1 = wave_sum_xor(t1);
    t2 = wave_sum_xor(t2);
    if (lane == 0) { red[wave] = t1; red[4 + wave] = t2; }
    __syncthreads();
    if (threadIdx.x == 0) pt0[gr] = make_float2(((red[0] + red[1]) + red[2]) + red[3], ((red[4] + red[5]) + red[6]) + red[7]);
}

// dst[i] += sum over the N rows of src[row][i], i < width.  A workgroup owns 16 consecutive i; thread (s, i) adds the rows s, s + 16,
// ... in order, and the 16 class sums are added as a fixed tree
__global__ void __launch_bounds__(256) k_acre_rowsum(const float* __restrict__ src, int64_t N, int width, float* __restrict__ dst) {
    __shared__ float part[16][17];
    const int il = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int i = (int)blockIdx.x * 16 + il;
    float v = 0.0f;
    if (i < width)
        for (int64_t row = s; row < N; row += 16) v += src[row * width + i];
    part[s][il] = v;
    __syncthreads();
    if (s == 0 && i < width) {
        float q[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) q[k] = part[k][il];
#pragma unroll
        for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
            for (int k = 0; k < w; ++k) q[k] = q[k] + q[k + w];
        dst[i] += q[0];
    }
}

// one wave: bn0's two sums per direction over the rows' partials -> t0[d], g_bn0
__global__ void __launch_bounds__(64) k_acre_bn0_fin(AcArgs a, const float2* __restrict__ pt0, float2* __restrict__ t0, float* __restrict__ g_w0,
                                                     float* __restrict__ g_b0) {
    const int lane = threadIdx.x;
    for (int d = 0; d < a.dirs; ++d) {
        float s1 = 0.0f, s2 = 0.0f;
        for (int64_t b = lane; b < a.n; b += 64) { const float2 v = pt0[(int64_t)d * a.n + b]; s1 += v.x; s2 += v.y; }
        s1 = wave_sum_xor(s1);
        s2 = wave_sum_xor(s2);
        if (lane == 0) { t0[d] = make_float2(s1, s2); g_w0[0] += s2; g_b0[0] += s1; }
    }
}

// one workgroup per row: bn0's backward of dy0 -> dent[row][j] (j < K) | drel[row][j - K]
__global__ void __launch_bounds__(256) k_acre_dcomb(AcArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                    const float* __restrict__ dimg, const float2* __restrict__ t0, float* __restrict__ dent,
                                                    float* __restrict__ drel) {
    const int64_t gr = blockIdx.x;
    const int d = (int)(gr / a.n);
    const float* __restrict__ st = tail_stats<AcTail>(a, d);
    const float* __restrict__ er = a.ent + e[gr] * a.K;
    const float* __restrict__ rr = a.rel + r[gr] * a.K;
    const float inv = 1.0f / ((float)a.n * (float)a.HW);
    const float mean0 = st[0], rstd0 = st[1];
    const float2 T = t0[d];
    for (int j = threadIdx.x; j < a.HW; j += 256) {
        const float xh = (ac_comb(a, er, rr, j) - mean0) * rstd0;
        const float v = (a.w0[0] * rstd0) * (dimg[gr * a.HW + j] - T.x * inv - xh * (T.y * inv));
        if (j < a.K) dent[gr * a.K + j] = v;
        else drel[gr * a.K + j - a.K] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the parallel way
// (kernels k_acrp_*; everything before z_1 and after c is the serial way's.)  A PAIR is (row, channel): pair p = row C + ch, M = N C of
// them; the stored layers [N, F] are [M, 400].  The gate c[p] = g_in[p] gate_w^T + gate_b has g_in[p] = [y0[row] | z_1[p] | z_2[p] | z_3[p]]:
// the y0 block of the contraction is the same for the C pairs of a row, so it is formed once per row (yg [N, 400], gate_b included) and
// added in the epilogue of the pairs' product, whose contraction is then 1200.
constexpr int kApNB = 2;            // column blocks of 16 per wave of k_acrp_gate: a workgroup owns 64 rows x 128 columns
constexpr int kApGW = 4 * kAcHW;    // row length of gate_w
constexpr int kApSub = 32;          // contraction length of one accumulation chain of k_acrp_gate
constexpr int kApPJ = (kAcHW + 63) / 64;   // positions lane + 64 j of a lane of k_acrp_conv_bwd
constexpr int kApPB = 5;            // position blocks of 16 per wave of k_acrp_gate_gw: 25 = 5 x 5
static_assert(kAcHW / 16 == kApPB * kApPB && kAcLS > kAcHW, "gate tiles, zero slot");
enum { kGateY0 = 0, kGateZ = 1, kGateDres = 2, kGateDz = 3 };

// y0d[row][pix] = bn0(img) * m0 as ac_load_y0 forms it: the A operand of the y0 block of the gate (kGateY0) and the B operand of the y0
// block of its weight gradient, which would otherwise draw the mask per use
__global__ void __launch_bounds__(256) k_acrp_y0(AcArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r, float* __restrict__ y0d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n * a.dirs * kAcHW) return;
    const int64_t gr = i / kAcHW;
    const int pix = (int)(i - gr * kAcHW);
    const float* __restrict__ st = tail_stats<AcTail>(a, (int)(gr / a.n));
    const float mean0 = st[0], g0 = st[1] * a.w0[0], b0 = a.b0[0];
    y0d[i] = ((ac_comb(a, a.ent + e[gr] * a.K, a.rel + r[gr] * a.K, pix) - mean0) * g0 + b0) * tail_factor(a, 0, pix, gr);
}

// out[m][col] = sum_k A[m][k] B[k][col] on v_mfma_f32_16x16x4_f32, grid (ceil(M / 64), ceil(cols / 128)): the A tile of 64 m x 128 k is
// staged in LDS as k_acre_fc stages it, wave w owns the column blocks (4 blockIdx.y + w) kApNB + {0, 1}, B comes from gate_w directly.
//   kGateY0    m = row,  A = y0d (src),                    k < 400,  B[k][pos] = gate_w[pos][k],        yg[row][pos] = . + gate_b[pos]
//   kGateZ     m = pair, A = [z_1 | z_2 | z_3][pair] (src), k < 1200, B[k][pos] = gate_w[pos][400 + k],  c[pair][pos] = . + yg[row][pos] (add)
//   kGateDres  m = row,  A = sum_ch dc (src),              k < 400,  B[k][q] = gate_w[k][q],            dres[row][q]
//   kGateDz    m = pair, A = dc (src),                     k < 400,  B[k][col] = gate_w[k][400 + col],  dz_i[pair][q], col = 400 i + q < 1200
// The three layers of src (kGateZ) and of out (kGateDz) lie M x 400 floats apart.
template <int MODE>
__global__ void __launch_bounds__(256) k_acrp_gate(AcArgs a, const float* __restrict__ gw, const float* __restrict__ gb,
                                                   const float* __restrict__ src, const float* __restrict__ add, float* __restrict__ out) {
    __shared__ float As[kTailKC * kTailStride];
    constexpr bool PAIRS = MODE == kGateZ || MODE == kGateDz, FWD = MODE == kGateY0 || MODE == kGateZ;
    constexpr int KT = MODE == kGateZ ? 3 * kAcHW : kAcHW, COLS = MODE == kGateDz ? 3 * kAcHW : kAcHW, OFF = PAIRS ? kAcHW : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int64_t M = a.n * a.dirs * (PAIRS ? a.C : 1), m0 = (int64_t)blockIdx.x * kTailRows, LAYER = M * kAcHW;
    int col[kApNB];
    bool live[kApNB];
#pragma unroll
    for (int nb = 0; nb < kApNB; ++nb) {
        const int ct = ((int)blockIdx.y * 4 + wave) * kApNB + nb;
        live[nb] = 16 * ct < COLS;   // (wave-uniform)
        col[nb] = live[nb] ? 16 * ct + l : 0;
    }
    // two levels of accumulation: a chain of v_mfma_f32_16x16x4_f32 over kApSub k, then added to the total.  One chain over the gate's
    // 1600 terms carries about four times the rounding error of this order, and c feeds batch norms that amplify it
    f32x4v acc[4][kApNB], sub[4][kApNB];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < kApNB; ++nb) acc[mb][nb] = sub[mb][nb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < KT; k0 += kTailKC) {
        const int kn = min(kTailKC, KT - k0), kn4 = (kn + 3) & ~3;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kTailKC * kTailRows; idx += 256) {
            const int kl = idx & (kTailKC - 1), rl = idx >> 7;   // consecutive threads: consecutive k of one m
            if (kl >= kn4) continue;
            float v = 0.0f;
            if (m0 + rl < M && kl < kn) {
                const int64_t m = m0 + rl;
                const int k = k0 + kl;
                if constexpr (MODE == kGateZ) v = src[(int64_t)(k / kAcHW) * LAYER + m * kAcHW + k % kAcHW];
                else v = src[m * kAcHW + k];
            }
            As[kl * kTailStride + 4 * (rl & 15) + (rl >> 4)] = v;
        }
        __syncthreads();
        if (live[0])
            for (int s0 = 0; s0 < kn4; s0 += kApSub) {
                const int ns = min(kApSub, kn4 - s0) / 4;   // steps of this chain: all of its B operands are requested before the first product
                float b[kApSub / 4][kApNB];
#pragma unroll
                for (int i = 0; i < kApSub / 4; ++i) {
                    const int k = min(k0 + s0 + 4 * i + g, KT - 1);   // (rows of As beyond the chunk are zero)
#pragma unroll
                    for (int nb = 0; nb < kApNB; ++nb) b[i][nb] = FWD ? gw[(int64_t)col[nb] * kApGW + OFF + k] : gw[(int64_t)k * kApGW + OFF + col[nb]];
                }
#pragma unroll
                for (int i = 0; i < kApSub / 4; ++i) {
                    if (i >= ns) continue;
                    float av[4];
                    read_blocks<4>(&As[(s0 + 4 * i + g) * kTailStride], l, av);
#pragma unroll
                    for (int nb = 0; nb < kApNB; ++nb)
                        if (live[nb])
#pragma unroll
                            for (int mb = 0; mb < 4; ++mb) sub[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], b[i][nb], sub[mb][nb], 0, 0, 0);
                }
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                    for (int nb = 0; nb < kApNB; ++nb) {
                        acc[mb][nb] += sub[mb][nb];
                        sub[mb][nb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
                    }
            }
    }
#pragma unroll
    for (int nb = 0; nb < kApNB; ++nb) {
        if (!live[nb]) continue;
        const int c = col[nb];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t m = m0 + 16 * mb + 4 * g + q;
                if (m >= M) continue;
                const float v = acc[mb][nb][q];
                if constexpr (MODE == kGateY0) out[m * kAcHW + c] = v + gb[c];
                else if constexpr (MODE == kGateZ) out[m * kAcHW + c] = v + add[(m / a.C) * kAcHW + c];
                else if constexpr (MODE == kGateDres) out[m * kAcHW + c] = v;
                else out[(int64_t)(c / kAcHW) * LAYER + m * kAcHW + c % kAcHW] = v;
            }
    }
}

// dcs[row][pos] = sum over the channels, ascending, of dc[row][ch][pos]: the A operand of kGateDres and of the y0 block of g_gate_w, and
// (through k_acre_rowsum) g_gate_b
__global__ void __launch_bounds__(256) k_acrp_chsum(AcArgs a, const float* __restrict__ dc, float* __restrict__ dcs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n * a.dirs * kAcHW) return;
    const int64_t gr = i / kAcHW;
    const int pos = (int)(i - gr * kAcHW);
    float s = 0.0f;
    for (int ch = 0; ch < a.C; ++ch) s += dc[gr * a.F + (int64_t)ch * kAcHW + pos];
    dcs[i] = s;
}

// the gate's weight gradient, the contraction read from global memory as k_acre_fc_gw reads it.  grid (q tiles / 4, 5, splits): wave w owns
// the 16 q of tile 4 blockIdx.x + w for the 80 positions of blockIdx.y (5 accumulator blocks).
//   ZB = false  the y0 block: g_gate_w[pos][q] += sum over the rows, ascending, of dcs[row][pos] y0d[row][q], q < 400 (z = y0d)
//   ZB = true   the z blocks: part[split][pos][col] = sum over the split's pairs [split per, ...), ascending, of dc[pair][pos]
//               z_i[pair][q], col = 400 i + q < 1200; k_acrp_gw_fin adds the splits in order
template <bool ZB>
__global__ void __launch_bounds__(256) k_acrp_gate_gw(AcArgs a, const float* __restrict__ dcx, const float* __restrict__ z, int64_t per,
                                                      float* __restrict__ out) {
    constexpr int QT = (ZB ? 3 : 1) * kAcHW / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int qt = (int)blockIdx.x * 4 + wave;
    if (qt >= QT) return;   // (wave-uniform)
    const int64_t M = a.n * a.dirs * (ZB ? a.C : 1), lo = (int64_t)blockIdx.z * per, hi = min(M, lo + per);
    const int p0 = 16 * kApPB * (int)blockIdx.y;
    const float* __restrict__ zl = z + (int64_t)(qt / (kAcHW / 16)) * M * kAcHW + 16 * (qt % (kAcHW / 16)) + l;   // (ZB = false: z = y0d, one layer)
    f32x4v acc[kApPB];
#pragma unroll
    for (int kb = 0; kb < kApPB; ++kb) acc[kb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t m0 = lo; m0 < hi; m0 += 4) {
        const int64_t m = m0 + g;
        const bool ok = m < hi;
        const int64_t mc = ok ? m : hi - 1;
        const float bv = ok ? zl[mc * kAcHW] : 0.0f;
        const float* __restrict__ dp = dcx + mc * kAcHW + p0 + l;
#pragma unroll
        for (int kb = 0; kb < kApPB; ++kb) acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? dp[16 * kb] : 0.0f, bv, acc[kb], 0, 0, 0);
    }
#pragma unroll
    for (int kb = 0; kb < kApPB; ++kb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int pos = p0 + 16 * kb + 4 * g + q;
            if constexpr (ZB) out[((int64_t)blockIdx.z * kAcHW + pos) * (3 * kAcHW) + 16 * qt + l] = acc[kb][q];
            else out[(int64_t)pos * kApGW + 16 * qt + l] += acc[kb][q];
        }
}

// g_gate_w[pos][400 + col] += the partial tiles of k_acrp_gate_gw<true> in split order
__global__ void __launch_bounds__(256) k_acrp_gw_fin(const float* __restrict__ part, int splits, float* __restrict__ g_gw) {
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= kAcHW * 3 * kAcHW) return;
    float s = 0.0f;
    for (int sp = 0; sp < splits; ++sp) s += part[(int64_t)sp * (kAcHW * 3 * kAcHW) + i];
    g_gw[(int64_t)(i / (3 * kAcHW)) * kApGW + kAcHW + i % (3 * kAcHW)] += s;
}

// one workgroup per row: the backward of the three 1 -> C convolutions of y0, the layers i = 0, 1, 2 in turn through ONE dz buffer in
// LDS.  The layer's tap table (a tap in the padding points at a zero slot) sits in LDS, the shifted y0 of a lane's positions in
// registers.  Per layer, as k_acre_c1_bwd: one wave per channel o, gwp[i][row][o 9 + t] = sum_pos dz_i[o, pos] y0[pos + tap t] and
// gbp[i][row][o] = sum_pos dz_i[o, pos]; then a thread per pixel adds conv_i^T dz_i (o ascending) to the pixel's register.  At the end
// dy0 = (the three layers' sum, i ascending, + dres) * m0 -> dimg[row][400]; (sum dy0, sum dy0 xh0) -> pt0[row]
__global__ void __launch_bounds__(256) k_acrp_conv_bwd(AcArgs a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                       const float* __restrict__ dz, const float* __restrict__ dres, float* __restrict__ gwp,
                                                       float* __restrict__ gbp, float* __restrict__ dimg, float2* __restrict__ pt0) {
    __shared__ float dzs[kAcMaxC * kAcLS];
    __shared__ float y0s[kAcHW + 1];
    __shared__ int tap[9 * kAcHW];
    __shared__ float wl[kAcMaxC * 9];
    __shared__ float red[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t gr = blockIdx.x, N = a.n * a.dirs;
    const float* __restrict__ st = tail_stats<AcTail>(a, (int)(gr / a.n));
    const int C = a.C;
    if (threadIdx.x < C) dzs[threadIdx.x * kAcLS + kAcHW] = 0.0f;   // a zero behind each channel's 400 values (the stride leaves room)
    if (threadIdx.x == 0) y0s[kAcHW] = 0.0f;                        // ... and behind y0's
    ac_load_y0(a, st, e, r, gr, y0s);
    float acc[2] = {0.0f, 0.0f};   // pixels threadIdx.x and threadIdx.x + 256
#pragma unroll 1
    for (int i = 0; i < 3; ++i) {
        const int d = a.dil[i];
        if (i) __syncthreads();   // every thread is done with the previous layer's dzs and wl
        for (int j = threadIdx.x; j < 9 * C; j += 256) wl[j] = a.cw[i][j];
        for (int j = threadIdx.x; j < 9 * kAcHW; j += 256) {   // the layer's tap table; in the padding: the zero slot
            const int q = ac_tap(j % kAcHW, j / kAcHW, d);
            tap[j] = q >= 0 ? q : kAcHW;
        }
        ac_load_layer(a, dz + (int64_t)i * N * a.F, gr, dzs);
        float ys[9][kApPJ];   // y0 at tap t of the lane's positions lane + 64 j: the same for every channel of the layer
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < kApPJ; ++j) ys[t][j] = y0s[lane + 64 * j < kAcHW ? tap[t * kAcHW + lane + 64 * j] : kAcHW];
        for (int o = wave; o < C; o += 4) {
            const float* __restrict__ drow = dzs + o * kAcLS;
            float dv[kApPJ], sb = 0.0f;
#pragma unroll
            for (int j = 0; j < kApPJ; ++j) {
                dv[j] = lane + 64 * j < kAcHW ? drow[lane + 64 * j] : 0.0f;
                sb += dv[j];
            }
            sb = wave_sum_xor(sb);
            if (lane == 0 && gbp) gbp[((int64_t)i * N + gr) * C + o] = sb;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                float s = 0.0f;
#pragma unroll
                for (int j = 0; j < kApPJ; ++j) s += dv[j] * ys[t][j];
                s = wave_sum_xor(s);
                if (lane == 0) gwp[((int64_t)i * N + gr) * (9 * C) + o * 9 + t] = s;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int pix = threadIdx.x + 256 * j;
            if (pix >= kAcHW) continue;
            int sp[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) sp[t] = tap[(8 - t) * kAcHW + pix];   // pix - tap t; in the padding: the channel's zero slot
            float v = 0.0f;
            for (int o = 0; o < C; ++o) {
                float s = 0.0f;
#pragma unroll
                for (int t = 0; t < 9; ++t) s += wl[o * 9 + t] * dzs[o * kAcLS + sp[t]];
                v += s;
            }
            acc[j] += v;
        }
    }
    const float mean0 = st[0], rstd0 = st[1];
    const float* __restrict__ er = a.ent + e[gr] * a.K;
    const float* __restrict__ rr = a.rel + r[gr] * a.K;
    float t1 = 0.0f, t2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int pix = threadIdx.x + 256 * j;
        if (pix >= kAcHW) continue;
        const float v = (acc[j] + dres[gr * kAcHW + pix]) * tail_factor(a, 0, pix, gr);
        dimg[gr * kAcHW + pix] = v;
        t1 += v;
        t2 += v * ((ac_comb(a, er, rr, pix) - mean0) * rstd0);
    }
    t1 = wave_sum_xor(t1);
    t2 = wave_sum_xor(t2);
    if (lane == 0) { red[wave] = t1; red[4 + wave] = t2; }
    __syncthreads();
    if (threadIdx.x == 0) pt0[gr] = make_float2(((red[0] + red[1]) + red[2]) + red[3], ((red[4] + red[5]) + red[6]) + red[7]);
}

// ------------------------------------------------------------------------------------------------------------------ host side
int AcTail::check(const kge_acre_desc* d, const char* who, bool grads) {
    if (!d) { set_error("%s: null descriptor", who); return -1; }
    const void* t[] = {d->bias, d->ent, d->rel, d->bn0_w, d->bn0_b, d->bn1_w, d->bn1_b, d->bn2_w, d->bn2_b, d->fc_w, d->fc_b,
                       d->conv1_w, d->conv2_w, d->conv3_w, d->bn0_mean, d->bn0_var, d->bn1_mean, d->bn1_var, d->bn2_mean, d->bn2_var};
    for (const void* p : t)
        if (!p) { set_error("%s: null tables (the parameters of the way and the six running buffers are all required)", who); return -1; }
    if (d->tot_entity <= 0 || d->tot_relation <= 0 || d->hidden_size <= 0 || d->in_channels <= 0) {
        set_error("%s: tot_entity, tot_relation, hidden_size and in_channels must be positive (got %lld, %lld, %d, %d)", who,
                  (long long)d->tot_entity, (long long)d->tot_relation, d->hidden_size, d->in_channels);
        return -1;
    }
    if (d->hidden_size != kAcK) {
        set_error("%s: hidden_size = %d must be 200 (the model views every embedding as 10 x 20)", who, d->hidden_size);
        return -1;
    }
    if (d->way != 0 && d->way != 1) { set_error("%s: way = %d must be 0 (serial) or 1 (parallel)", who, d->way); return -1; }
    const int dil[3] = {d->first_atrous, d->second_atrous, d->third_atrous};
    for (int i = 0; i < 3; ++i)
        if (dil[i] < 1 || dil[i] > KGE_ACRE_MAX_ATROUS) {
            set_error("%s: dilation %d = %d must be in [1, %d]", who, i + 1, dil[i], KGE_ACRE_MAX_ATROUS);
            return -1;
        }
    if (d->in_channels > kAcMaxC) {
        set_error("%s: in_channels = %d exceeds %d (a layer of in_channels x 400 values is held in LDS)", who, d->in_channels, kAcMaxC);
        return -1;
    }
    const bool cb = d->conv1_b && d->conv2_b && d->conv3_b, nocb = !d->conv1_b && !d->conv2_b && !d->conv3_b;
    if (d->acre_bias ? !cb : !nocb) {
        set_error("%s: the convolution bias pointers must all be set with acre_bias = 1 and all be NULL with acre_bias = 0", who);
        return -1;
    }
    const bool gate = d->gate_w && d->gate_b, nogate = !d->gate_w && !d->gate_b;
    if (d->way ? !gate : !nogate) {
        set_error("%s: the gate pointers must both be set in the parallel way and both be NULL in the serial way", who);
        return -1;
    }
    if (tail_check_rates(d, who)) return -1;
    if (grads) {
        const void* g[] = {d->g_bias, d->g_ent, d->g_rel, d->g_bn0_w, d->g_bn0_b, d->g_bn1_w, d->g_bn1_b, d->g_bn2_w, d->g_bn2_b, d->g_fc_w,
                           d->g_fc_b, d->g_conv1_w, d->g_conv2_w, d->g_conv3_w};
        for (const void* q : g)
            if (!q) { set_error("%s: null gradient buffers (one per parameter of the way is required)", who); return -1; }
        if ((d->acre_bias && (!d->g_conv1_b || !d->g_conv2_b || !d->g_conv3_b)) || (d->way == 1 && (!d->g_gate_w || !d->g_gate_b))) {
            set_error("%s: null gradient buffers (one per parameter of the way is required)", who);
            return -1;
        }
    }
    return 0;
}

static int ac_ss(const kge_acre_desc* d) { return 2 + 2 * d->in_channels + 2 * kAcK; }
static int ac_f(const kge_acre_desc* d) { return d->in_channels * kAcHW; }

static AcArgs ac_args(const kge_acre_desc* d, int64_t n, int dirs, int64_t row0, float* stats) {
    AcArgs a{};
    tail_fill(a, d, n, dirs, row0, stats);
    a.ent = d->ent; a.rel = d->rel; a.w0 = d->bn0_w; a.b0 = d->bn0_b;
    a.cw[0] = d->conv1_w; a.cw[1] = d->conv2_w; a.cw[2] = d->conv3_w;
    a.cb[0] = d->conv1_b; a.cb[1] = d->conv2_b; a.cb[2] = d->conv3_b;
    a.dil[0] = d->first_atrous; a.dil[1] = d->second_atrous; a.dil[2] = d->third_atrous;
    a.K = kAcK; a.HW = kAcHW; a.C = d->in_channels; a.F = ac_f(d);
    a.SS = ac_ss(d); a.o1 = 2; a.o2 = 2 + 2 * a.C;
    return a;
}

// saved (floats): c [N, F] | z1 [N, F] | z2 [N, F] | u [N, K] | m1f [N, C] | stats [dirs][2 + 2C + 2K]; the parallel way keeps a
// third layer, c | z_1 | z_2 | z_3 | u | m1f | stats: the z_i are saved, not recomputed (the backward reads them twice, as the
// gate's input and never as a convolution's)
static int ac_layers(const kge_acre_desc* d) { return d->way ? 4 : 3; }
size_t AcTail::saved_floats(const kge_acre_desc* d, int64_t n, int dirs) {
    return (size_t)dirs * ((size_t)n * ((size_t)ac_layers(d) * ac_f(d) + kAcK + d->in_channels) + ac_ss(d));
}
static size_t ac_part_bytes(const kge_acre_desc* d, size_t N) { return align256(N * (d->in_channels > 2 ? d->in_channels : 2) * sizeof(float2)); }
// forward: row partials float2 [N, max(C, 2)] (bn0's are double2 [N]) | upart [splits, N, K] | the parallel way: yg [N, 400] | y0d [N, 400]
static size_t ac_upart_bytes(const kge_acre_desc* d, int64_t n, int dirs) {
    return tail_upart_bytes(kAcK, ac_f(d), n, dirs);
}
size_t AcTail::fwd_bytes(const kge_acre_desc* d, int64_t n, int dirs) {
    const size_t N = (size_t)n * dirs;
    return ac_part_bytes(d, N) + ac_upart_bytes(d, n, dirs) + (d->way ? 2 * align256(N * kAcHW * sizeof(float)) : 0);
}
// backward: du [N, K] | dy1 = dc [N, F] | dza [N, F] | dzb [N, F] | part1 float2 [N, C] | sums float2 [dirs, C] | gwp3 [N, 9 C C] |
// gwp2 [N, 9 C C] | gwp1 [N, 9 C] | gbp [3][N, C] | dimg [N, 400] | dent [N, K] | drel [N, K] | pt0 float2 [N] | t0 float2 [dirs]
struct AcBwdPlan {
    size_t du, dy1, dza, dzb, part1, sums, gwp3, gwp2, gwp1, gbp, dimg, dent, drel, pt0, t0, total;
};
static AcBwdPlan ac_bwd_plan(const kge_acre_desc* d, int64_t n, int dirs) {
    const size_t N = (size_t)n * dirs, C = (size_t)d->in_channels, F = (size_t)ac_f(d);
    AcBwdPlan p{};
    p.du = 0;
    p.dy1 = p.du + align256(N * kAcK * sizeof(float));
    p.dza = p.dy1 + align256(N * F * sizeof(float));
    p.dzb = p.dza + align256(N * F * sizeof(float));
    p.part1 = p.dzb + align256(N * F * sizeof(float));
    p.sums = p.part1 + align256(N * C * sizeof(float2));
    p.gwp3 = p.sums + align256((size_t)dirs * C * sizeof(float2));
    p.gwp2 = p.gwp3 + align256(N * 9 * C * C * sizeof(float));
    p.gwp1 = p.gwp2 + align256(N * 9 * C * C * sizeof(float));
    p.gbp = p.gwp1 + align256(N * 9 * C * sizeof(float));
    p.dimg = p.gbp + 3 * align256(N * C * sizeof(float));
    p.dent = p.dimg + align256(N * kAcHW * sizeof(float));
    p.drel = p.dent + align256(N * kAcK * sizeof(float));
    p.pt0 = p.drel + align256(N * kAcK * sizeof(float));
    p.t0 = p.pt0 + align256(N * sizeof(float2));
    p.total = p.t0 + align256((size_t)dirs * sizeof(float2));
    return p;
}

// pairs of one split of the gate's weight gradient: a function of the shapes alone (the split order is the summation order), a
// multiple of 4, every split non-empty
static int64_t ap_gw_per(int64_t M) {
    int64_t splits = (M + 1023) / 1024;
    if (splits > 16) splits = 16;
    const int64_t per = ((M + splits - 1) / splits + 3) & ~(int64_t)3;
    return per;
}
static int ap_gw_splits(int64_t M) { return (int)((M + ap_gw_per(M) - 1) / ap_gw_per(M)); }

// backward of the parallel way: du [N, K] | dc [N, F] | dz [3][N, F] | part1 float2 [N, C] | sums float2 [dirs, C] | dcs [N, 400] |
// dres [N, 400] | y0d [N, 400] | gpart [splits][400][1200] | gwp [3][N, 9 C] | gbp [3][N, C] | dimg [N, 400] | dent [N, K] | drel [N, K] |
// pt0 float2 [N] | t0 float2 [dirs]
struct ApBwdPlan {
    size_t du, dc, dz, part1, sums, dcs, dres, y0d, gpart, gwp, gbp, dimg, dent, drel, pt0, t0, total;
};
static ApBwdPlan ap_bwd_plan(const kge_acre_desc* d, int64_t n, int dirs) {
    const size_t N = (size_t)n * dirs, C = (size_t)d->in_channels, F = (size_t)ac_f(d);
    ApBwdPlan p{};
    p.du = 0;
    p.dc = p.du + align256(N * kAcK * sizeof(float));
    p.dz = p.dc + align256(N * F * sizeof(float));
    p.part1 = p.dz + align256(3 * N * F * sizeof(float));
    p.sums = p.part1 + align256(N * C * sizeof(float2));
    p.dcs = p.sums + align256((size_t)dirs * C * sizeof(float2));
    p.dres = p.dcs + align256(N * kAcHW * sizeof(float));
    p.y0d = p.dres + align256(N * kAcHW * sizeof(float));
    p.gpart = p.y0d + align256(N * kAcHW * sizeof(float));
    p.gwp = p.gpart + align256((size_t)ap_gw_splits((int64_t)(N * C)) * kAcHW * 3 * kAcHW * sizeof(float));
    p.gbp = p.gwp + align256(3 * N * 9 * C * sizeof(float));
    p.dimg = p.gbp + align256(3 * N * C * sizeof(float));
    p.dent = p.dimg + align256(N * kAcHW * sizeof(float));
    p.drel = p.dent + align256(N * kAcK * sizeof(float));
    p.pt0 = p.drel + align256(N * kAcK * sizeof(float));
    p.t0 = p.pt0 + align256(N * sizeof(float2));
    p.total = p.t0 + align256((size_t)dirs * sizeof(float2));
    return p;
}
size_t AcTail::bwd_bytes(const kge_acre_desc* d, int64_t n, int dirs) {
    return d->way ? ap_bwd_plan(d, n, dirs).total : ac_bwd_plan(d, n, dirs).total;
}

int AcTail::forward(const kge_acre_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int, int64_t row0, float* x, float* saved,
                    void* ws, hipStream_t st) {
    const int64_t N = n * dirs;
    const int C = d->in_channels, F = ac_f(d);
    float *c = saved, *z1 = c + N * F, *z2 = z1 + N * F, *u = z2 + (ac_layers(d) - 2) * N * F, *m1f = u + N * kAcK, *stats = m1f + N * C;
    const AcArgs a = ac_args(d, n, dirs, row0, stats);
    float2* part = (float2*)ws;
    float* upart = (float*)((char*)ws + ac_part_bytes(d, (size_t)N));
    const bool train = d->train != 0;
    const int chan_groups = (C + 3) / 4 < 8 ? (C + 3) / 4 : 8;
    if (train) {
        hipLaunchKernelGGL(k_acre_row_stats, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, a, e, r, (double2*)ws);
        hipLaunchKernelGGL(k_acre_bn0_stats, dim3(1), dim3(64), 0, st, a, (const double2*)ws, d->eps[0], d->momentum[0], d->bn0_mean, d->bn0_var);
    } else {
        hipLaunchKernelGGL(k_acre_stats_eval, dim3((unsigned)((1 + C + kAcK + 255) / 256)), dim3(256), 0, st, a, d->eps[0], d->eps[1], d->eps[2],
                           d->bn0_mean, d->bn0_var, d->bn1_mean, d->bn1_var, d->bn2_mean, d->bn2_var);
    }
    if (d->way) {
        // z_i = conv_i(y0) into three consecutive layers; yg = y0's block of the gate once per row; c = the pairs' product + yg
        float* yg = (float*)((char*)ws + ac_part_bytes(d, (size_t)N) + ac_upart_bytes(d, n, dirs));
        float* y0d = (float*)((char*)yg + align256((size_t)N * kAcHW * sizeof(float)));
        hipLaunchKernelGGL(k_acrp_y0, dim3((unsigned)((N * kAcHW + 255) / 256)), dim3(256), 0, st, a, e, r, y0d);
        for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(k_acre_conv1, dim3((unsigned)N), dim3(256), 0, st, a, i, e, r, z1 + i * N * F);
        hipLaunchKernelGGL((k_acrp_gate<kGateY0>), dim3((unsigned)((N + kTailRows - 1) / kTailRows), 4), dim3(256), 0, st, a, d->gate_w, d->gate_b,
                           (const float*)y0d, (const float*)nullptr, yg);
        hipLaunchKernelGGL((k_acrp_gate<kGateZ>), dim3((unsigned)((N * C + kTailRows - 1) / kTailRows), 4), dim3(256), 0, st, a, d->gate_w,
                           d->gate_b, (const float*)z1, (const float*)yg, c);
        if (int rc = check_launch("k_acre_row_stats / k_acre_bn0_stats / k_acrp_y0 / k_acre_conv1 / k_acrp_gate")) return rc;
    } else {
        hipLaunchKernelGGL(k_acre_conv1, dim3((unsigned)N), dim3(256), 0, st, a, 0, e, r, z1);
        hipLaunchKernelGGL((k_acre_cc<false>), dim3((unsigned)N), dim3(256), 0, st, a, 1, 0, e, r, z1, z2);
        hipLaunchKernelGGL((k_acre_cc<false>), dim3((unsigned)N), dim3(256), 0, st, a, 2, 1, e, r, z2, c);
        if (int rc = check_launch("k_acre_row_stats / k_acre_bn0_stats / k_acre_conv1 / k_acre_cc")) return rc;
    }
    if (train) {
        hipLaunchKernelGGL(k_acre_c_stats, dim3((unsigned)N, (unsigned)chan_groups), dim3(256), 0, st, a, c, part, m1f);
        hipLaunchKernelGGL(k_acre_bn_fin, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, st, a, part, C, C, 1, kAcHW, a.o1, a.o1 + C, d->eps[1],
                           d->momentum[1], d->bn1_mean, d->bn1_var);
    }
    return tail_fc_forward<AcTail>(d, a, c, m1f, upart, u, x, st);   // (its check covers k_acre_c_stats and k_acre_bn_fin)
}

// the parallel way's backward: the serial tail down to dc, the gate (weight, bias and input gradients), the three convolutions of y0 at
// once, then bn0's backward and the scatter as in the serial way
static int ap_backward(const kge_acre_desc* d, const AcArgs& a, const int64_t* e, const int64_t* r, int64_t n, int dirs, const float* dx,
                       const float* c, const float* z, const float* u, const float* m1f, void* ws, hipStream_t st) {
    const int64_t N = n * dirs;
    const int C = d->in_channels;
    const int64_t M = N * C;
    const ApBwdPlan p = ap_bwd_plan(d, n, dirs);
    char* w = (char*)ws;
    float *du = (float*)(w + p.du), *dc = (float*)(w + p.dc), *dz = (float*)(w + p.dz), *dcs = (float*)(w + p.dcs), *dres = (float*)(w + p.dres);
    float *y0d = (float*)(w + p.y0d), *gpart = (float*)(w + p.gpart), *gwp = (float*)(w + p.gwp), *gbp = d->acre_bias ? (float*)(w + p.gbp) : nullptr;
    float *dimg = (float*)(w + p.dimg), *dent = (float*)(w + p.dent), *drel = (float*)(w + p.drel);
    float2 *part1 = (float2*)(w + p.part1), *sums = (float2*)(w + p.sums), *pt0 = (float2*)(w + p.pt0), *t0 = (float2*)(w + p.t0);
    const int chan_groups = (C + 3) / 4 < 8 ? (C + 3) / 4 : 8;
    if (int rc = tail_backward<AcTail>(d, a, dx, c, m1f, u, du, dc, part1, sums, chan_groups, st)) return rc;
    hipLaunchKernelGGL(k_acre_bn1_dc, dim3((unsigned)N, (unsigned)chan_groups), dim3(256), 0, st, a, c, dc, sums);
    if (int rc = check_launch("k_acre_bn1_part / k_acre_bn1_bwd_fin / k_acre_bn1_dc")) return rc;
    // the gate: dcs = the channel sum of dc; g_gate_b; g_gate_w's y0 block over the rows and its z blocks over the pairs in splits;
    // dres = dcs gate_w[:, :400] and dz_i = dc gate_w[:, 400 (i + 1) ...]
    const int64_t per = ap_gw_per(M);
    const int splits = ap_gw_splits(M);
    hipLaunchKernelGGL(k_acrp_chsum, dim3((unsigned)((N * kAcHW + 255) / 256)), dim3(256), 0, st, a, (const float*)dc, dcs);
    hipLaunchKernelGGL(k_acrp_y0, dim3((unsigned)((N * kAcHW + 255) / 256)), dim3(256), 0, st, a, e, r, y0d);
    hipLaunchKernelGGL(k_acre_rowsum, dim3((unsigned)((kAcHW + 15) / 16)), dim3(256), 0, st, dcs, N, kAcHW, d->g_gate_b);
    hipLaunchKernelGGL((k_acrp_gate_gw<false>), dim3((unsigned)((kAcHW / 16 + 3) / 4), kApPB, 1), dim3(256), 0, st, a, (const float*)dcs,
                       (const float*)y0d, N, d->g_gate_w);
    hipLaunchKernelGGL((k_acrp_gate_gw<true>), dim3((unsigned)((3 * kAcHW / 16 + 3) / 4), kApPB, (unsigned)splits), dim3(256), 0, st, a,
                       (const float*)dc, z, per, gpart);
    hipLaunchKernelGGL(k_acrp_gw_fin, dim3((unsigned)((kAcHW * 3 * kAcHW + 255) / 256)), dim3(256), 0, st, (const float*)gpart, splits, d->g_gate_w);
    if (int rc = check_launch("k_acrp_chsum / k_acrp_y0 / k_acre_rowsum / k_acrp_gate_gw / k_acrp_gw_fin")) return rc;
    hipLaunchKernelGGL((k_acrp_gate<kGateDres>), dim3((unsigned)((N + kTailRows - 1) / kTailRows), 4), dim3(256), 0, st, a, d->gate_w, d->gate_b,
                       (const float*)dcs, (const float*)nullptr, dres);
    hipLaunchKernelGGL((k_acrp_gate<kGateDz>), dim3((unsigned)((M + kTailRows - 1) / kTailRows), (unsigned)((3 * kAcHW + 127) / 128)), dim3(256), 0, st, a,
                       d->gate_w, d->gate_b, (const float*)dc, (const float*)nullptr, dz);
    hipLaunchKernelGGL(k_acrp_conv_bwd, dim3((unsigned)N), dim3(256), 0, st, a, e, r, (const float*)dz, (const float*)dres, gwp, gbp, dimg, pt0);
    if (int rc = check_launch("k_acrp_gate / k_acrp_conv_bwd")) return rc;
    float* gw[3] = {d->g_conv1_w, d->g_conv2_w, d->g_conv3_w};
    float* gb[3] = {d->g_conv1_b, d->g_conv2_b, d->g_conv3_b};
    for (int i = 0; i < 3; ++i) {
        hipLaunchKernelGGL(k_acre_rowsum, dim3((unsigned)((9 * C + 15) / 16)), dim3(256), 0, st, gwp + (int64_t)i * N * 9 * C, N, 9 * C, gw[i]);
        if (gbp) hipLaunchKernelGGL(k_acre_rowsum, dim3((unsigned)((C + 15) / 16)), dim3(256), 0, st, gbp + (int64_t)i * N * C, N, C, gb[i]);
    }
    hipLaunchKernelGGL(k_acre_bn0_fin, dim3(1), dim3(64), 0, st, a, pt0, t0, d->g_bn0_w, d->g_bn0_b);
    hipLaunchKernelGGL(k_acre_dcomb, dim3((unsigned)N), dim3(256), 0, st, a, e, r, dimg, t0, dent, drel);
    if (int rc = check_launch("k_acre_rowsum / k_acre_bn0_fin / k_acre_dcomb")) return rc;
    tail_scatter<AcTail>(e, N, kAcK, dent, kAcK, d->g_ent, st);   // (every id is scattered, id 0 included: no padding_idx)
    tail_scatter<AcTail>(r, N, kAcK, drel, kAcK, d->g_rel, st);
    return check_launch("k_acre_scatter");
}

int AcTail::backward(const kge_acre_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int, int64_t row0, const float* dx,
                     const float* saved, void* ws, hipStream_t st) {
    const int64_t N = n * dirs;
    const int C = d->in_channels, F = ac_f(d);
    const float *c = saved, *z1 = c + N * F, *z2 = z1 + N * F, *u = z2 + (ac_layers(d) - 2) * N * F, *m1f = u + N * kAcK;
    const AcArgs a = ac_args(d, n, dirs, row0, const_cast<float*>(m1f + N * C));
    if (d->way) return ap_backward(d, a, e, r, n, dirs, dx, c, z1, u, m1f, ws, st);
    const AcBwdPlan p = ac_bwd_plan(d, n, dirs);
    char* w = (char*)ws;
    float *du = (float*)(w + p.du), *dy1 = (float*)(w + p.dy1), *dza = (float*)(w + p.dza), *dzb = (float*)(w + p.dzb);
    float *gwp3 = (float*)(w + p.gwp3), *gwp2 = (float*)(w + p.gwp2), *gwp1 = (float*)(w + p.gwp1), *dimg = (float*)(w + p.dimg);
    float *dent = (float*)(w + p.dent), *drel = (float*)(w + p.drel);
    const size_t gbs = align256((size_t)N * C * sizeof(float));
    float* gbp[3] = {nullptr, nullptr, nullptr};
    if (d->acre_bias)
        for (int i = 0; i < 3; ++i) gbp[i] = (float*)(w + p.gbp + i * gbs);
    float2 *part1 = (float2*)(w + p.part1), *sums = (float2*)(w + p.sums), *pt0 = (float2*)(w + p.pt0), *t0 = (float2*)(w + p.t0);
    const int chan_groups = (C + 3) / 4 < 8 ? (C + 3) / 4 : 8;
    if (int rc = tail_backward<AcTail>(d, a, dx, c, m1f, u, du, dy1, part1, sums, chan_groups, st)) return rc;
    hipLaunchKernelGGL(k_acre_bn1_dc, dim3((unsigned)N, (unsigned)chan_groups), dim3(256), 0, st, a, c, dy1, sums);
    if (int rc = check_launch("k_acre_bn1_part / k_acre_bn1_bwd_fin / k_acre_bn1_dc")) return rc;
    // dz3 = dc: conv3's partials against z2, dz2 = conv3^T dz3; conv2's against z1, dz1 = conv2^T dz2; conv1's against y0
    hipLaunchKernelGGL(k_acre_cc_gw, dim3((unsigned)N), dim3(256), 0, st, a, 2, dy1, z2, gwp3, gbp[2]);
    hipLaunchKernelGGL((k_acre_cc<true>), dim3((unsigned)N), dim3(256), 0, st, a, 2, 0, e, r, dy1, dza);
    hipLaunchKernelGGL(k_acre_cc_gw, dim3((unsigned)N), dim3(256), 0, st, a, 1, dza, z1, gwp2, gbp[1]);
    hipLaunchKernelGGL((k_acre_cc<true>), dim3((unsigned)N), dim3(256), 0, st, a, 1, 0, e, r, dza, dzb);
    hipLaunchKernelGGL(k_acre_c1_bwd, dim3((unsigned)N), dim3(256), 0, st, a, 0, e, r, dzb, dy1, gwp1, gbp[0], dimg, pt0);
    if (int rc = check_launch("k_acre_cc_gw / k_acre_cc / k_acre_c1_bwd")) return rc;
    const int w9 = 9 * C * C;
    hipLaunchKernelGGL(k_acre_rowsum, dim3((unsigned)((w9 + 15) / 16)), dim3(256), 0, st, gwp3, N, w9, d->g_conv3_w);
    hipLaunchKernelGGL(k_acre_rowsum, dim3((unsigned)((w9 + 15) / 16)), dim3(256), 0, st, gwp2, N, w9, d->g_conv2_w);
    hipLaunchKernelGGL(k_acre_rowsum, dim3((unsigned)((9 * C + 15) / 16)), dim3(256), 0, st, gwp1, N, 9 * C, d->g_conv1_w);
    if (d->acre_bias) {
        float* gb[3] = {d->g_conv1_b, d->g_conv2_b, d->g_conv3_b};
        for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(k_acre_rowsum, dim3((unsigned)((C + 15) / 16)), dim3(256), 0, st, gbp[i], N, C, gb[i]);
    }
    hipLaunchKernelGGL(k_acre_bn0_fin, dim3(1), dim3(64), 0, st, a, pt0, t0, d->g_bn0_w, d->g_bn0_b);
    hipLaunchKernelGGL(k_acre_dcomb, dim3((unsigned)N), dim3(256), 0, st, a, e, r, dimg, t0, dent, drel);
    if (int rc = check_launch("k_acre_rowsum / k_acre_bn0_fin / k_acre_dcomb")) return rc;
    tail_scatter<AcTail>(e, N, kAcK, dent, kAcK, d->g_ent, st);   // (every id is scattered, id 0 included: no padding_idx)
    tail_scatter<AcTail>(r, N, kAcK, drel, kAcK, d->g_rel, st);
    return check_launch("k_acre_scatter");
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_acre_saved_floats(const kge_acre_desc* d, int64_t n) {
    return tail_bytes<AcTail, AcTail::saved_floats>("kge_acre_saved_floats", d, n);
}

size_t kge_acre_body_forward_workspace_bytes(const kge_acre_desc* d, int64_t n) {
    return tail_bytes<AcTail, AcTail::fwd_bytes>("kge_acre_body_forward_workspace_bytes", d, n);
}

int kge_acre_body_forward(const kge_acre_desc* d, const int64_t* e, const int64_t* r, int64_t n, int64_t row0, float* x, float* saved,
                          void* workspace, size_t workspace_bytes, void* stream) {
    return tail_body_forward<AcTail>("kge_acre_body_forward", d, e, r, n, 0, row0, x, saved, workspace, workspace_bytes, stream);
}

size_t kge_acre_body_backward_workspace_bytes(const kge_acre_desc* d, int64_t n) {
    return tail_bytes<AcTail, AcTail::bwd_bytes>("kge_acre_body_backward_workspace_bytes", d, n);
}

int kge_acre_body_backward(const kge_acre_desc* d, const int64_t* e, const int64_t* r, int64_t n, int64_t row0, const float* dx,
                           const float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    return tail_body_backward<AcTail>("kge_acre_body_backward", d, e, r, n, 0, row0, dx, saved, workspace, workspace_bytes, stream);
}

size_t kge_acre_train_bce_workspace_bytes(const kge_acre_desc* d, int64_t batch, int64_t n_hr, int64_t n_tr) {
    return tail_train_bce_bytes<AcTail>("kge_acre_train_bce_workspace_bytes", d, batch, n_hr, n_tr);
}

int kge_acre_train_bce(const kge_acre_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t batch, const int64_t* hr_off,
                       const int32_t* hr_ids, int64_t n_hr, const int64_t* tr_off, const int32_t* tr_ids, int64_t n_tr, float label_smoothing,
                       void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    return tail_train_bce<AcTail>("kge_acre_train_bce", d, h, r, t, batch, hr_off, hr_ids, n_hr, tr_off, tr_ids, n_tr, label_smoothing, workspace,
                                  workspace_bytes, loss, stream);
}

size_t kge_acre_eval_ranks_workspace_bytes(const kge_acre_desc* d, int64_t n) {
    return tail_eval_ranks_bytes<AcTail>("kge_acre_eval_ranks_workspace_bytes", d, n);
}

int kge_acre_eval_ranks(const kge_acre_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                        const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks, int32_t* ties,
                        void* stream) {
    return tail_eval_ranks<AcTail>("kge_acre_eval_ranks", d, triples, n, tail_off, tail_ids, head_off, head_ids, workspace, workspace_bytes, ranks,
                                   ties, stream);
}

}  // extern "C"
