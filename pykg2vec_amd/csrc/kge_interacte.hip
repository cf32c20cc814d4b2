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
//     u      = A fc_w^T + fc_b,  x = relu(bn2(u * m2))            the shared tail (kge_conv_tail.h); bn2 in BOTH forms (eval: running statistics)
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
//     the shared tail         du, g_bn2, g_fc_b, g_fc, dy1 = (du x fc_w) * m1 [bn1 > 0] and the two sums of bn1's backward with g_bn1
//     k_interacte_conv_gw     per row and permutation: dc from dy1 (in place) and the filter sums gfp[row, p, f, t] = sum_pos dc[pos]
//                             y0[pos shifted by tap t]
//     k_interacte_conv_dx     per row and permutation: the circular correlation of dc with the flipped filters into dy0 (times m0)
//     k_interacte_small_fin   g_conv_filt[f, t] += the (row, p) partials in index order -- the sum over p of the shared filter -- and
//                             bn0's two sums per permutation with g_bn0
//     k_interacte_dcomb       d comb[b, j] = sum_p (bn0's backward of dy0)[b, p, inv_perm[p, j]], p ascending -> dent | drel rows
//     k_interacte_scatter   adds the rows to g_ent[e] / g_rel[r] in row order (no atomics: the wave of the FIRST row that names an
//                             id owns it); every id is scattered, id 0 included (no padding_idx)
// No kernel of this file uses atomics.
//
// The dropout draw is the shared one (kge_projection.h spells the Philox counters out), with
//     site 0: elem = p H W + pixel in [0, 2K P);   site 1: elem = channel in [0, C), one draw per row and channel;   site 2: elem = j in [0, K)
//     row = row0 + position in the call's row list.  The fused step numbers the h rows 0 .. B-1 and the t rows B .. 2B-1.
#include "kge_conv_tail.h"

namespace kge {

constexpr int kItMaxK = KGE_INTERACTE_MAX_HIDDEN;    // K: the 2K pixels of a permutation, padded and as four channels of dc, in LDS (k_interacte_conv_gw / k_interacte_conv_dx)
constexpr int kItMaxKs = KGE_INTERACTE_MAX_KERNEL;   // ks: a filter's taps per wave in LDS
constexpr int kItMaxT = 128;                         // >= kItMaxKs^2
constexpr int kItPadMax = 6 * kItMaxK + 256;         // floats of the circularly padded image: (H + 2 pad)(W + 2 pad) with pad <= min(H, W, 5),
                                                     // H W <= 2 kItMaxK is at most 3 H W + 150 (W <= 5) or H W + 10 (H + W) + 100 (both > 5); it_check tests it
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

// the tail's policy (kge_conv_tail.h): F = C H W need not be a multiple of 16
struct ItTail : TailReluM1f<ItArgs> {
    using Desc = kge_interacte_desc;
    static constexpr const char* kBadArgs = "row0 + n below 2^32";
    static int check(const Desc* d, const char* who, bool grads);
    static int dim(const Desc* d) { return d->reshape_width * d->reshape_height; }
    static int64_t rel_rows(const Desc* d) { return d->tot_relation; }
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
KGE_CONV_TAIL_KERNELS(interacte, ItTail, false)

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
        if (train) v *= tail_factor(a, 0, p * a.HW + pix, gr);
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
    it_load_image(a, tail_stats<ItTail>(a, (int)(gr / a.n)), e, r, gr, p, TRAIN, pimg);
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
                m1f[gr * a.C + ch] = tail_factor(a, 1, ch, gr);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
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
    const float* __restrict__ st = tail_stats<ItTail>(a, d);
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
    const float* __restrict__ st = tail_stats<ItTail>(a, (int)(gr / a.n));
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
        const float v = accs[pix] * tail_factor(a, 0, p * a.HW + pix, gr);
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
    const float* __restrict__ st = tail_stats<ItTail>(a, d);
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

int ItTail::check(const kge_interacte_desc* d, const char* who, bool grads) {
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
    if (tail_check_rates(d, who)) return -1;
    if (grads) {
        const void* g[] = {d->g_bias, d->g_conv_filt, d->g_ent, d->g_rel, d->g_bn0_w, d->g_bn0_b, d->g_bn1_w, d->g_bn1_b, d->g_bn2_w, d->g_bn2_b,
                           d->g_fc_w, d->g_fc_b};
        for (const void* q : g)
            if (!q) { set_error("%s: null gradient buffers (all 12 are required)", who); return -1; }
    }
    return 0;
}

static ItArgs it_args(const kge_interacte_desc* d, int64_t n, int dirs, int64_t row0, float* stats) {
    const ItShape s = it_shape(d);
    ItArgs a{};
    tail_fill(a, d, n, dirs, row0, stats);
    a.ent = d->ent; a.rel = d->rel; a.w0 = d->bn0_w; a.b0 = d->bn0_b; a.filt = d->conv_filt; a.perm = d->perm; a.inv = d->inv_perm;
    a.K = s.K; a.H = s.H; a.W = s.W; a.HW = s.HW; a.P = s.P; a.NF = s.NF; a.ks = s.ks; a.pad = s.pad; a.T = s.T; a.C = s.C; a.F = s.F;
    a.Wp = s.Wp; a.PS = s.PS; a.SS = s.SS; a.o1 = 2 * s.P; a.o2 = 2 * s.P + 2 * s.C;
    return a;
}

// saved (floats): conv [N, F] | u [N, K] | m1f [N, C] | stats [dirs][2P + 2C + 2K]
size_t ItTail::saved_floats(const kge_interacte_desc* d, int64_t n, int dirs) {
    const ItShape s = it_shape(d);
    return (size_t)dirs * ((size_t)n * ((size_t)s.F + s.K + s.C) + s.SS);
}
// forward: row partials float2 [N, max(C, 1)] | upart [splits, N, K]
size_t ItTail::fwd_bytes(const kge_interacte_desc* d, int64_t n, int dirs) {
    const ItShape s = it_shape(d);
    const size_t N = (size_t)n * dirs;
    return align256(N * s.C * sizeof(float2)) + tail_upart_bytes(s.K, s.F, n, dirs);
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
size_t ItTail::bwd_bytes(const kge_interacte_desc* d, int64_t n, int dirs) { return it_bwd_plan(d, n, dirs).total; }

int ItTail::forward(const kge_interacte_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int, int64_t row0, float* x, float* saved,
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
    return tail_fc_forward<ItTail>(d, a, conv, m1f, upart, u, x, st);
}

int ItTail::backward(const kge_interacte_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int, int64_t row0, const float* dx,
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
    const int chan_groups = (s.C + 3) / 4 < 16 ? (s.C + 3) / 4 : 16;
    if (int rc = tail_backward<ItTail>(d, a, dx, conv, m1f, u, du, dy1, part1, sums, chan_groups, st)) return rc;
    hipLaunchKernelGGL(k_interacte_conv_gw, dim3((unsigned)(N * s.P)), dim3(256), 0, st, a, e, r, conv, dy1, sums, gfp);
    hipLaunchKernelGGL(k_interacte_conv_dx, dim3((unsigned)(N * s.P)), dim3(256), 0, st, a, e, r, dy1, dimg, pt0);
    if (int rc = check_launch("k_interacte_bn1_part / k_interacte_bn1_bwd_fin / k_interacte_conv_gw / k_interacte_conv_dx")) return rc;
    hipLaunchKernelGGL(k_interacte_small_fin, dim3((unsigned)((s.NF * s.T + s.P + 3) / 4)), dim3(256), 0, st, a, gfp, pt0, t0, d->g_conv_filt,
                       d->g_bn0_w, d->g_bn0_b);
    hipLaunchKernelGGL(k_interacte_dcomb, dim3((unsigned)N), dim3(256), 0, st, a, e, r, dimg, t0, dent, drel);
    if (int rc = check_launch("k_interacte_small_fin / k_interacte_dcomb")) return rc;
    tail_scatter<ItTail>(e, N, s.K, dent, s.K, d->g_ent, st);   // (every id is scattered, id 0 included: no padding_idx)
    tail_scatter<ItTail>(r, N, s.K, drel, s.K, d->g_rel, st);
    return check_launch("k_interacte_scatter");
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_interacte_saved_floats(const kge_interacte_desc* d, int64_t n) {
    return tail_bytes<ItTail, ItTail::saved_floats>("kge_interacte_saved_floats", d, n);
}

size_t kge_interacte_body_forward_workspace_bytes(const kge_interacte_desc* d, int64_t n) {
    return tail_bytes<ItTail, ItTail::fwd_bytes>("kge_interacte_body_forward_workspace_bytes", d, n);
}

int kge_interacte_body_forward(const kge_interacte_desc* d, const int64_t* e, const int64_t* r, int64_t n, int64_t row0, float* x, float* saved,
                               void* workspace, size_t workspace_bytes, void* stream) {
    return tail_body_forward<ItTail>("kge_interacte_body_forward", d, e, r, n, 0, row0, x, saved, workspace, workspace_bytes, stream);
}

size_t kge_interacte_body_backward_workspace_bytes(const kge_interacte_desc* d, int64_t n) {
    return tail_bytes<ItTail, ItTail::bwd_bytes>("kge_interacte_body_backward_workspace_bytes", d, n);
}

int kge_interacte_body_backward(const kge_interacte_desc* d, const int64_t* e, const int64_t* r, int64_t n, int64_t row0, const float* dx,
                                const float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    return tail_body_backward<ItTail>("kge_interacte_body_backward", d, e, r, n, 0, row0, dx, saved, workspace, workspace_bytes, stream);
}

size_t kge_interacte_train_bce_workspace_bytes(const kge_interacte_desc* d, int64_t batch, int64_t n_hr, int64_t n_tr) {
    return tail_train_bce_bytes<ItTail>("kge_interacte_train_bce_workspace_bytes", d, batch, n_hr, n_tr);
}

int kge_interacte_train_bce(const kge_interacte_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t batch, const int64_t* hr_off,
                            const int32_t* hr_ids, int64_t n_hr, const int64_t* tr_off, const int32_t* tr_ids, int64_t n_tr, float label_smoothing,
                            void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    return tail_train_bce<ItTail>("kge_interacte_train_bce", d, h, r, t, batch, hr_off, hr_ids, n_hr, tr_off, tr_ids, n_tr, label_smoothing, workspace,
                                  workspace_bytes, loss, stream);
}

size_t kge_interacte_eval_ranks_workspace_bytes(const kge_interacte_desc* d, int64_t n) {
    return tail_eval_ranks_bytes<ItTail>("kge_interacte_eval_ranks_workspace_bytes", d, n);
}

int kge_interacte_eval_ranks(const kge_interacte_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                             const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks, int32_t* ties,
                             void* stream) {
    return tail_eval_ranks<ItTail>("kge_interacte_eval_ranks", d, triples, n, tail_off, tail_ids, head_off, head_ids, workspace, workspace_bytes, ranks,
                                   ties, stream);
}

}  // extern "C"
