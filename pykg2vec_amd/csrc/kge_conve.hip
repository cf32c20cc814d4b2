// kge_conve.hip -- the body of ConvE (models/projection.py:12-125) in front of the 1-N head of kge_head.hip.
// For a row with entity e and relation r on side s (0 = "tail" direction, 1 = "head": relation row r + tot_relation), k = hidden_size,
// h1 = hidden_size_1, h2 = k / h1, image H x W = 2 h2 x h1, conv output OH x OW = (H - 2) x (W - 2), F = 32 OH OW:
//     img  = [ent[e] ; rel[r']]                                   2k pixels, row-major, the entity half first
//     y0   = bn0(img) * m0                                        one channel; input dropout, site 0
//     c    = conv3x3(y0) + conv_b                                 32 channels, VALU from the image in LDS (k_conve_conv); STORED once
//     A    = relu(bn1(c)) * m1                                    feature-map dropout, site 1: a whole channel of a row; never stored
//     u    = A fc_w^T + fc_b,  x = relu(bn2(u * m2))               the shared tail (kge_conv_tail.h); eval form: x = relu(u), no bn2
// Training form: every batch norm normalises with the statistics of ITS DIRECTION's n rows and updates its running buffers, the
// tail direction first.  Statistics are fixed-order sums: per-row (count, mean, M2) partials (deviations about the row's own mean),
// combined over the rows in index order with the equal-count form of Chan's rule (mean of the means; M2 = sum M2_b + cnt sum
// (mean_b - mean)^2).  Eval form (template parameter TRAIN = false): running statistics, no bn2, no draws.
//
// A call works on `dirs` directions of n rows each (body entry points: 1; fused step and rank pass: 2, sides 0 and 1) in the SAME
// launches: the direction is a range of the row axis, row d n + b belongs to direction d.
//
// Backward (training form only), dx the gradient at x:
//     the shared tail     du, g_bn2, g_fc_b, g_fc, dy1 = (du x fc_w) * m1 * [bn1 > 0] and the two sums of bn1's backward with g_bn1
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
#include "kge_conv_tail.h"

namespace kge {

constexpr int kCvMaxK = KGE_CONVE_MAX_HIDDEN;       // hidden_size limit: the image (2k floats) and four channels of dc (< 8k floats) fit 48 KB of LDS
constexpr int kCvCh = 32;           // conv2d_1's output channels

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

// the tail's policy (kge_conv_tail.h)
struct CvTail {
    using Args = CvArgs;
    using Desc = kge_conve_desc;
    static constexpr bool kClamp = false, kEvalBn2 = false;   // F = 32 P is a multiple of 16
    static constexpr const char* kBadArgs = "side must be 0 or 1, row0 + n below 2^32";
    __host__ __device__ static int K(const Args& a) { return a.k; }
    __host__ __device__ static int F(const Args& a) { return a.F; }
    __host__ __device__ static int C(const Args&) { return kCvCh; }
    __host__ __device__ static int E(const Args& a) { return a.P; }
    __host__ __device__ static int SS(const Args& a) { return 66 + 2 * a.k; }
    __host__ __device__ static int o1(const Args&) { return 2; }
    __host__ __device__ static int o2(const Args&) { return 66; }
    // A[row][f] = relu(bn1(conv)) * m1, formed from the stored conv output
    template <bool TRAIN>
    __device__ __forceinline__ static float feature(const Args& a, const float* __restrict__ st, const float* __restrict__ conv, const float*, int64_t gr,
                                                    int f) {
        const int ch = f / a.P;
        float v = fmaxf((conv[gr * a.F + f] - st[2 + ch]) * (st[34 + ch] * a.w1[ch]) + a.b1[ch], 0.0f);
        if constexpr (TRAIN) v *= tail_factor(a, 1, ch, gr);
        return v;
    }
    struct Bn1 {
        float mean, gain, bias;
    };
    __device__ __forceinline__ static Bn1 bn1_chan(const Args& a, const float* __restrict__ st, int ch) {
        return Bn1{st[2 + ch], st[34 + ch] * a.w1[ch], a.b1[ch]};
    }
    __device__ __forceinline__ static float dy1(const Args& a, const Bn1& bn, const float* __restrict__ conv, const float*, int64_t gr, int f, int ch,
                                                float acc) {
        const float y1 = (conv[gr * a.F + f] - bn.mean) * bn.gain + bn.bias;
        return y1 > 0.0f ? acc * tail_factor(a, 1, ch, gr) : 0.0f;
    }
    static int check(const Desc* d, const char* who, bool grads);
    static int dim(const Desc* d) { return d->hidden_size; }
    static int64_t rel_rows(const Desc* d) { return d->tot_relation; }   // (the rows read are r + side * tot_relation of a [2R, k] table)
    static const float* bias(const Desc* d) { return d->b; }
    static float* g_bias(const Desc* d) { return d->g_b; }
    static size_t saved_floats(const Desc* d, int64_t n, int dirs);
    static size_t fwd_bytes(const Desc* d, int64_t n, int dirs);
    static size_t bwd_bytes(const Desc* d, int64_t n, int dirs);
    static int forward(const Desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int side0, int64_t row0, float* x, float* saved, void* ws,
                       hipStream_t st);
    static int backward(const Desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int side0, int64_t row0, const float* dx,
                        const float* saved, void* ws, hipStream_t st);
};
KGE_CONV_TAIL_KERNELS(conve, CvTail, false)

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
    const float* __restrict__ st = tail_stats<CvTail>(a, d);
    const float mean0 = st[0], g0 = st[1] * a.w0[0], b0 = a.b0[0];
    for (int p = threadIdx.x; p < 2 * a.k; p += 256) {
        float v = (cv_pixel(a, e, r, gr, d, p) - mean0) * g0 + b0;
        if constexpr (TRAIN) v *= tail_factor(a, 0, p, gr);
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

// ------------------------------------------------------------------------------------------------------------------ backward
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
    const float* __restrict__ st = tail_stats<CvTail>(a, d);
    const float mean0 = st[0], rstd0 = st[1], g0 = rstd0 * a.w0[0], b0 = a.b0[0];
    for (int p = threadIdx.x; p < np; p += 256) img[p] = ((cv_pixel(a, e, r, gr, d, p) - mean0) * g0 + b0) * tail_factor(a, 0, p, gr);
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
        const float v = accs[p] * tail_factor(a, 0, p, gr);
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
    const float* __restrict__ st = tail_stats<CvTail>(a, d);
    const float mean0 = st[0], rstd0 = st[1], gain = a.w0[0] * rstd0;
    const float2 T = t0[d];
    const float inv = 1.0f / ((float)a.n * (float)np);
    for (int p = lane; p < np; p += 64) {
        const float xh = (cv_pixel(a, e, r, gr, d, p) - mean0) * rstd0;
        dy0[gr * np + p] = gain * (dy0[gr * np + p] - T.x * inv - xh * (T.y * inv));
    }
    if (lane == 0) rp[gr] = r[gr] + (int64_t)(a.side0 + d) * a.R;
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

int CvTail::check(const kge_conve_desc* d, const char* who, bool grads) {
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
    if (tail_check_rates(d, who)) return -1;
    if (grads) {
        const void* g[] = {d->g_ent, d->g_rel, d->g_b, d->g_bn0_w, d->g_bn0_b, d->g_conv_w, d->g_conv_b, d->g_bn1_w, d->g_bn1_b, d->g_fc_w, d->g_fc_b,
                           d->g_bn2_w, d->g_bn2_b};
        for (const void* q : g)
            if (!q) { set_error("%s: null gradient buffers (all 13 are required)", who); return -1; }
    }
    return 0;
}

static CvArgs cv_args(const kge_conve_desc* d, int64_t n, int dirs, int side0, int64_t row0, float* stats) {
    const CvShape s = cv_shape(d);
    CvArgs a{};
    tail_fill(a, d, n, dirs, row0, stats);
    a.ent = d->ent; a.rel = d->rel; a.w0 = d->bn0_w; a.b0 = d->bn0_b; a.cw = d->conv_w; a.cb = d->conv_b;
    a.k = s.k; a.W = s.W; a.P = s.P; a.OW = s.OW; a.F = s.F;
    a.side0 = side0; a.R = d->tot_relation;
    return a;
}

// saved (floats): conv [N, F] | u [N, k] | stats [dirs][66 + 2k]
size_t CvTail::saved_floats(const kge_conve_desc* d, int64_t n, int dirs) {
    const CvShape s = cv_shape(d);
    return (size_t)dirs * ((size_t)n * ((size_t)s.F + s.k) + 66 + 2 * (size_t)s.k);
}
// forward: row partials float2 [N, 32] | upart [splits, N, k]
size_t CvTail::fwd_bytes(const kge_conve_desc* d, int64_t n, int dirs) {
    const CvShape s = cv_shape(d);
    const size_t N = (size_t)n * dirs;
    return align256(N * kCvCh * sizeof(float2)) + tail_upart_bytes(s.k, s.F, n, dirs);
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
size_t CvTail::bwd_bytes(const kge_conve_desc* d, int64_t n, int dirs) { return cv_bwd_plan(d, n, dirs).total; }

int CvTail::forward(const kge_conve_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int side0, int64_t row0, float* x, float* saved,
                    void* ws, hipStream_t st) {
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
        hipLaunchKernelGGL(k_conve_bn_fin, dim3(1), dim3(256), 0, st, a, part, 1, 1, 1, 2 * s.k, 0, 1, d->eps[0], d->momentum[0], d->bn0_mean, d->bn0_var);
        hipLaunchKernelGGL((k_conve_conv<true>), dim3((unsigned)N), dim3(256), 0, st, a, e, r, conv, part);
        if (int rc = check_launch("k_conve_img_stats / k_conve_bn_fin / k_conve_conv")) return rc;
        hipLaunchKernelGGL(k_conve_bn_fin, dim3(kCvCh / 4), dim3(256), 0, st, a, part, kCvCh, kCvCh, 1, s.P, 2, 34, d->eps[1], d->momentum[1],
                           d->bn1_mean, d->bn1_var);
    } else {
        hipLaunchKernelGGL(k_conve_stats_eval, dim3(1), dim3(64), 0, st, a, d->eps[0], d->eps[1], d->bn0_mean, d->bn0_var, d->bn1_mean, d->bn1_var);
        hipLaunchKernelGGL((k_conve_conv<false>), dim3((unsigned)N), dim3(256), 0, st, a, e, r, conv, part);
    }
    return tail_fc_forward<CvTail>(d, a, conv, nullptr, upart, u, x, st);
}

int CvTail::backward(const kge_conve_desc* d, const int64_t* e, const int64_t* r, int64_t n, int dirs, int side0, int64_t row0, const float* dx,
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
    const unsigned row_blocks = (unsigned)((N + 3) / 4);
    if (int rc = tail_backward<CvTail>(d, a, dx, conv, nullptr, u, du, dy1, part1, sums, 1, st)) return rc;
    hipLaunchKernelGGL(k_conve_conv_bwd, dim3((unsigned)N), dim3(256), 0, st, a, e, r, conv, dy1, sums, pcw, dy0, pt0);
    if (int rc = check_launch("k_conve_bn1_part / k_conve_bn1_bwd_fin / k_conve_conv_bwd")) return rc;
    hipLaunchKernelGGL(k_conve_small_fin, dim3((kCvCh * 10 + 1 + 3) / 4), dim3(256), 0, st, a, pcw, pt0, t0, d->g_conv_w, d->g_conv_b, d->g_bn0_w,
                       d->g_bn0_b);
    hipLaunchKernelGGL(k_conve_dimg, dim3(row_blocks), dim3(256), 0, st, a, e, r, t0, dy0, rp);
    tail_scatter<CvTail>(e, N, s.k, dy0, 2 * s.k, d->g_ent, st);
    tail_scatter<CvTail>(rp, N, s.k, dy0 + s.k, 2 * s.k, d->g_rel, st);
    return check_launch("k_conve_small_fin / k_conve_dimg / k_conve_scatter");
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_conve_saved_floats(const kge_conve_desc* d, int64_t n) {
    return tail_bytes<CvTail, CvTail::saved_floats>("kge_conve_saved_floats", d, n);
}

size_t kge_conve_body_forward_workspace_bytes(const kge_conve_desc* d, int64_t n) {
    return tail_bytes<CvTail, CvTail::fwd_bytes>("kge_conve_body_forward_workspace_bytes", d, n);
}

int kge_conve_body_forward(const kge_conve_desc* d, const int64_t* e, const int64_t* r, int64_t n, int32_t side, int64_t row0, float* x,
                           float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    return tail_body_forward<CvTail>("kge_conve_body_forward", d, e, r, n, side, row0, x, saved, workspace, workspace_bytes, stream);
}

size_t kge_conve_body_backward_workspace_bytes(const kge_conve_desc* d, int64_t n) {
    return tail_bytes<CvTail, CvTail::bwd_bytes>("kge_conve_body_backward_workspace_bytes", d, n);
}

int kge_conve_body_backward(const kge_conve_desc* d, const int64_t* e, const int64_t* r, int64_t n, int32_t side, int64_t row0, const float* dx,
                            const float* saved, void* workspace, size_t workspace_bytes, void* stream) {
    return tail_body_backward<CvTail>("kge_conve_body_backward", d, e, r, n, side, row0, dx, saved, workspace, workspace_bytes, stream);
}

size_t kge_conve_train_bce_workspace_bytes(const kge_conve_desc* d, int64_t batch, int64_t n_hr, int64_t n_tr) {
    return tail_train_bce_bytes<CvTail>("kge_conve_train_bce_workspace_bytes", d, batch, n_hr, n_tr);
}

int kge_conve_train_bce(const kge_conve_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t batch, const int64_t* hr_off,
                        const int32_t* hr_ids, int64_t n_hr, const int64_t* tr_off, const int32_t* tr_ids, int64_t n_tr, float label_smoothing,
                        void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    return tail_train_bce<CvTail>("kge_conve_train_bce", d, h, r, t, batch, hr_off, hr_ids, n_hr, tr_off, tr_ids, n_tr, label_smoothing, workspace,
                                  workspace_bytes, loss, stream);
}

size_t kge_conve_eval_ranks_workspace_bytes(const kge_conve_desc* d, int64_t n) {
    return tail_eval_ranks_bytes<CvTail>("kge_conve_eval_ranks_workspace_bytes", d, n);
}

int kge_conve_eval_ranks(const kge_conve_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                         const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks, int32_t* ties,
                         void* stream) {
    return tail_eval_ranks<CvTail>("kge_conve_eval_ranks", d, triples, n, tail_off, tail_ids, head_off, head_ids, workspace, workspace_bytes, ranks,
                                   ties, stream);
}

}  // extern "C"
