// kge_convkb.hip -- ConvKB (pointwise.py:241-318) as the reference executes it: convolutions over the stacked [h; r; t] rows followed
// directly by fc1, with no activation and no dropout in between.  The score is therefore affine in the three gathered rows,
//     preds(h, r, t) = c0 + <A_h, ent[h]> + <A_r, rel[r]> + <A_t, ent[t]>,
// with A_* (dim floats each) and c0 functions of the filters and fc1 alone (k_convkb_collapse; formulas in DESIGN.md section 14).  The
// filters are fixed inputs (conv_list is a plain list: they are in no optimiser), so the trainable tensors are ent, rel, fc1.weight and
// fc1.bias.  With g_i = d loss / d preds_i:
//     d ent[h_i] += g_i A_h,  d ent[t_i] += g_i A_t,  d rel[r_i] += g_i A_r            (float atomics, shared rows of a bundle pre-summed)
//     d fc1.bias = G = sum_i g_i
//     d fc1.weight[f W + off_j + p] = conv_j.bias[f] G + sum_row sum_c conv_j.weight[f, 0, row, c] X_row[p + c],  X_h = sum_i g_i ent[h_i] ...
// X_h, X_r, X_t and G are ORDERED sums: every lane group of the step owns one slice of `part` and adds its bundles' shares in program
// order; k_convkb_finish adds the slices in slice order -- the fc1 gradient is bit-identical run to run.
//
// Every kernel walks its rows in chunks of the lane group (lane gl holds elements gl, gl + G, ...): nothing live grows with dim.
//
//   collapse             one thread per element of A_h | A_r | A_t, one wave for c0
//   forward              one lane group per triple
//   step / backward      one lane group per bundle (a positive and its neg_rate corruptions, or `bundle` explicit rows; backward:
//                        single rows with the caller's d loss / d preds): pass 1 leaves member k's coefficient in lane k, pass 2
//                        scatters coefficient * A_* and adds coefficient * row into the group's slice of X
//   finish, fc1 grad     the slices in order; one thread per fc1.weight element
//   rank                 P_h[e] = <A_h, ent[e]>, P_t[e] = <A_t, ent[e]>, P_r[r] = <A_r, rel[r]> in one pass over the tables; the energy of
//                        candidate e is the fp32 sum q + P[e] with q the query's constant; the sweep stores it, the rank counts on it
#include "kge_row_kernels.h"
#include "kge_projection.h"   // ws_check

namespace kge {

constexpr int kCkbMaxSlices = 1024;   // lane groups of one step launch (= slices of the ordered partial sums)
constexpr int kCkbFinishWaves = 16;

struct CkbGeom {
    int k, F, nw, W;
    int s[KGE_CONVKB_MAX_WIDTHS];      // filter widths, conv_list order
    int off[KGE_CONVKB_MAX_WIDTHS];    // first output column of width j inside a filter's W columns
    int woff[KGE_CONVKB_MAX_WIDTHS];   // first float of conv_j.weight inside conv_w
};

// ---------------------------------------------------------------- collapse: A_h | A_r | A_t | c0
__global__ __launch_bounds__(kBlock) void k_convkb_collapse(CkbGeom g, const float* __restrict__ conv_w,
                                                            const float* __restrict__ conv_b, const float* __restrict__ fc_w,
                                                            const float* __restrict__ fc_b, float* __restrict__ out) {
    const int k = g.k;
    if (blockIdx.x == gridDim.x - 1) {   // c0: one wave, lane l takes the fc1 columns l, l + 64, ...; fixed order throughout
        if (threadIdx.x >= 64) return;
        float acc = 0.f;
        const int total = g.F * g.W;
        for (int idx = threadIdx.x; idx < total; idx += 64) {
            const int f = idx / g.W, q = idx - f * g.W;
            int j = 0;
            while (j + 1 < g.nw && q >= g.off[j + 1]) ++j;
            acc = fmaf(conv_b[j * g.F + f], fc_w[idx], acc);
        }
        acc = wave_sum(acc);
        if (threadIdx.x == 0) out[3 * k] = fc_b[0] + acc;
        return;
    }
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= 3 * k) return;
    const int row = i / k, d = i - row * k;
    float acc = 0.f;
    for (int j = 0; j < g.nw; ++j) {
        const int s = g.s[j], last = k - s;   // output columns 0 .. k - s
        for (int f = 0; f < g.F; ++f) {
            const float* w = conv_w + g.woff[j] + (f * 3 + row) * s;
            const float* v = fc_w + (int64_t)f * g.W + g.off[j];
            for (int c = 0; c < s; ++c) {
                const int p = d - c;
                if (p >= 0 && p <= last) acc = fmaf(w[c], v[p], acc);
            }
        }
    }
    out[i] = acc;
}

// ---------------------------------------------------------------- forward: one lane group per triple
struct CkbArgs {
    const float* ent; const float* rel;
    float* gent; float* grel;
    const float* A;     // A_h | A_r | A_t | c0
    float* part;        // [slices][3 k + 1]
    int k;
};

template <int G>
__device__ __forceinline__ float ckb_pred(const CkbArgs& a, int64_t h, int64_t r, int64_t t, int gl) {
    const int k = a.k;
    const float* eh = a.ent + h * k;
    const float* er = a.rel + r * k;
    const float* et = a.ent + t * k;
    float p = 0.f;
    for (int e = gl; e < k; e += G) p += a.A[e] * eh[e] + a.A[k + e] * er[e] + a.A[2 * k + e] * et[e];
    return gsum<G>(p) + a.A[3 * k];
}

template <int G>
__global__ __launch_bounds__(kBlock) void k_convkb_forward(CkbArgs a, const int64_t* __restrict__ h, const int64_t* __restrict__ r,
                                                           const int64_t* __restrict__ t, int64_t n, float* __restrict__ scores) {
    constexpr int GPB = kBlock / G;
    const int gl = threadIdx.x % G;
    for (int64_t i = (int64_t)blockIdx.x * GPB + threadIdx.x / G; i < n; i += (int64_t)gridDim.x * GPB) {
        const float p = ckb_pred<G>(a, h[i], r[i], t[i], gl);
        if (gl == 0) scores[i] = p;
    }
}

// coefficient * A into the row's gradient (atomics), coefficient * row into the group's slice (plain, this lane's own elements)
template <int G>
__device__ __forceinline__ void ckb_row(const float* __restrict__ A, const float* __restrict__ tab, float* __restrict__ gtab,
                                        float* __restrict__ X, int64_t row, int k, float c, int gl) {
    if (c == 0.f) return;   // group-uniform
    const float* x = tab + row * k;
    float* gx = gtab + row * k;
    for (int e = gl; e < k; e += G) {
        unsafeAtomicAdd(gx + e, c * A[e]);
        X[e] = fmaf(c, x[e], X[e]);
    }
}

// ---------------------------------------------------------------- fused pointwise-logistic step / backward: one lane group per bundle
// (SAMPLED: the sampler in front, no id arrays; otherwise explicit rows -- two instantiations, so neither keeps the other's arguments live)
template <int G, bool SAMPLED>
__global__ __launch_bounds__(kBlock) void k_convkb_step(CkbArgs a, const int64_t* __restrict__ h, const int64_t* __restrict__ r,
                                                        const int64_t* __restrict__ t, const int64_t* __restrict__ y,
                                                        const float* __restrict__ dscore, int64_t n, int bundle,
                                                        float* __restrict__ loss, FusedSampler fs) {
    constexpr int GPB = kBlock / G;
    const int gl = threadIdx.x % G;
    const int gbase = (threadIdx.x & 63) / G * G;
    const int k = a.k;
    constexpr bool sampled = SAMPLED;
    const int64_t s_start = (sampled && fs.cursor) ? fs.start + fs.cursor[0] : fs.start;
    const unsigned long long s_off = (sampled && fs.cursor) ? fs.offset + (unsigned long long)fs.cursor[1] : fs.offset;
    const float inv_n = 1.0f / (float)n;
    const int64_t nb = (n + bundle - 1) / bundle;
    const int64_t slice = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    float* X = a.part + slice * (3 * k + 1);
    for (int seg = 0; seg < 3; ++seg)   // (per segment: a lane clears exactly the elements it later adds into)
        for (int e = gl; e < k; e += G) X[seg * k + e] = 0.f;
    float acc = 0.f, gtot = 0.f;
    for (int64_t b = slice; b < nb; b += (int64_t)gridDim.x * GPB) {
        const int64_t i0 = b * bundle;
        const int nm = (int)(min(n, i0 + bundle) - i0);
        int64_t pos[3];
        int my_nh = 0, my_nt = 0;
        if constexpr (sampled) {
            const int64_t row = fs.perm[s_start + b];
            pos[0] = fs.triples[3 * row]; pos[1] = fs.triples[3 * row + 1]; pos[2] = fs.triples[3 * row + 2];
            if (gl < bundle - 1) {
                int64_t nh, nt;
                corrupt_one(pos[0], pos[1], pos[2], fs.E, fs.bern, fs.slots, fs.mask, fs.seed,
                            s_off + (unsigned long long)(b * (bundle - 1) + gl), nh, nt);
                my_nh = (int)nh; my_nt = (int)nt;
            }
        } else {
            pos[0] = h[i0]; pos[1] = r[i0]; pos[2] = t[i0];
        }
        auto member = [&](int m, int64_t& mh, int64_t& mr, int64_t& mt, float& my) {   // member m of the bundle (group-uniform m)
            if constexpr (sampled) {
                const int src = gbase + (m > 0 ? m - 1 : 0);
                const int nh = __shfl(my_nh, src, 64), nt = __shfl(my_nt, src, 64);
                mh = m == 0 ? pos[0] : (int64_t)nh; mr = pos[1]; mt = m == 0 ? pos[2] : (int64_t)nt;
                my = m == 0 ? 1.f : -1.f;
            } else {
                mh = h[i0 + m]; mr = r[i0 + m]; mt = t[i0 + m];
                my = y ? (float)y[i0 + m] : 0.f;
            }
        };
        // pass 1: member m's coefficient d(loss)/d(preds) in lane m
        float my_g = 0.f;
        for (int m = 0; m < nm; ++m) {
            if constexpr (!sampled) {
                if (dscore) {
                    if (gl == m) my_g = dscore[i0 + m];
                    continue;
                }
            }
            int64_t mh, mr, mt;
            float my;
            member(m, mh, mr, mt, my);
            const float x = my * ckb_pred<G>(a, mh, mr, mt, gl);
            if (gl == m) {
                acc += softplus_t(x) * inv_n;
                my_g = my * sigmoid_t(x) * inv_n;
            }
        }
        // pass 2: rows shared with the first member take the sum of their members' coefficients and scatter once, in a last round
        float ch = 0.f, cr = 0.f, ct = 0.f;
        for (int m = 0; m <= nm; ++m) {
            int64_t mh = pos[0], mr = pos[1], mt = pos[2];
            float gh = ch, gr = cr, gt = ct;
            if (m < nm) {
                float my;
                member(m, mh, mr, mt, my);
                const float g = __shfl(my_g, gbase + m, 64);
                gtot += g;
                gh = gr = gt = g;
                if (mh == pos[0]) { ch += g; gh = 0.f; }
                if (mr == pos[1]) { cr += g; gr = 0.f; }
                if (mt == pos[2]) { ct += g; gt = 0.f; }
            }
            ckb_row<G>(a.A, a.ent, a.gent, X, mh, k, gh, gl);
            ckb_row<G>(a.A + k, a.rel, a.grel, X + k, mr, k, gr, gl);
            ckb_row<G>(a.A + 2 * k, a.ent, a.gent, X + 2 * k, mt, k, gt, gl);
        }
    }
    if (gl == 0) X[3 * k] = gtot;
    if (loss) block_accumulate_loss<G>(gsum<G>(acc), gl, loss);
}

// X[e] = part[0][e] + part[1][e] + ... in slice order: wave w adds its run of consecutive slices, the runs are added in wave order
__global__ __launch_bounds__(64 * kCkbFinishWaves) void k_convkb_finish(const float* __restrict__ part, int slices, int width,
                                                                        float* __restrict__ X) {
    __shared__ float s_run[kCkbFinishWaves][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const int per = (slices + kCkbFinishWaves - 1) / kCkbFinishWaves;
    const int s0 = w * per, s1 = min(slices, s0 + per);
    float acc = 0.f;
    if (e < width)
        for (int s = s0; s < s1; ++s) acc += part[(int64_t)s * width + e];
    s_run[w][lane] = acc;
    __syncthreads();
    if (w == 0 && e < width) {
        float tot = s_run[0][lane];
#pragma unroll
        for (int q = 1; q < kCkbFinishWaves; ++q) tot += s_run[q][lane];
        X[e] = tot;
    }
}

// one thread per fc1.weight element; thread 0 also adds G to the fc1.bias gradient
__global__ __launch_bounds__(kBlock) void k_convkb_fc_grad(CkbGeom g, const float* __restrict__ conv_w, const float* __restrict__ conv_b,
                                                           const float* __restrict__ X, float* __restrict__ g_fc_w,
                                                           float* __restrict__ g_fc_b) {
    const int k = g.k;
    const float G_ = X[3 * k];
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx == 0) g_fc_b[0] += G_;
    if (idx >= g.F * g.W) return;
    const int f = idx / g.W, q = idx - f * g.W;
    int j = 0;
    while (j + 1 < g.nw && q >= g.off[j + 1]) ++j;
    const int p = q - g.off[j], s = g.s[j];
    float acc = conv_b[j * g.F + f] * G_;
    for (int row = 0; row < 3; ++row) {
        const float* w = conv_w + g.woff[j] + (f * 3 + row) * s;
        const float* x = X + row * k + p;
        for (int c = 0; c < s; ++c) acc = fmaf(w[c], x[c], acc);
    }
    g_fc_w[idx] += acc;
}

// ---------------------------------------------------------------- rank: projections, sweep rows, counts
// row i < E: P_h[i], P_t[i]; row E + i: P_r[i].  P = P_h [E] | P_t [E] | P_r [R]
template <int G>
__global__ __launch_bounds__(kBlock) void k_convkb_project(CkbArgs a, int64_t E, int64_t R, float* __restrict__ P) {
    constexpr int GPB = kBlock / G;
    const int gl = threadIdx.x % G;
    const int k = a.k;
    for (int64_t i = (int64_t)blockIdx.x * GPB + threadIdx.x / G; i < E + R; i += (int64_t)gridDim.x * GPB) {
        if (i < E) {
            const float* x = a.ent + i * k;
            float ph = 0.f, pt = 0.f;
            for (int e = gl; e < k; e += G) {
                const float v = x[e];
                ph = fmaf(a.A[e], v, ph);
                pt = fmaf(a.A[2 * k + e], v, pt);
            }
            gsum2<G>(ph, pt);
            if (gl == 0) { P[i] = ph; P[E + i] = pt; }
        } else {
            const float* x = a.rel + (i - E) * k;
            float pr = 0.f;
            for (int e = gl; e < k; e += G) pr = fmaf(a.A[k + e], x[e], pr);
            pr = gsum<G>(pr);
            if (gl == 0) P[2 * E + (i - E)] = pr;
        }
    }
}

// the constant of a sweep and the projection its candidates add: tail sweep (h, r, ?) / head sweep (?, r, t)
__device__ __forceinline__ float ckb_query(const float* __restrict__ P, float c0, int64_t E, const int64_t* __restrict__ trip, bool head,
                                           const float*& cand) {
    const float pr = P[2 * E + trip[1]];
    if (head) { cand = P; return (c0 + pr) + P[E + trip[2]]; }
    cand = P + E;
    return (c0 + P[trip[0]]) + pr;
}

// row i = the tail sweep (side 0) or the head sweep (side 1) of triple i
__global__ __launch_bounds__(kBlock) void k_convkb_sweep(const float* __restrict__ P, const float* __restrict__ A, int k, int64_t E,
                                                         const int64_t* __restrict__ triples, int64_t rows, int side,
                                                         float* __restrict__ scores) {
    const float c0 = A[3 * k];
    for (int64_t q = blockIdx.y; q < rows; q += gridDim.y) {
        const float* cand;
        const float qv = ckb_query(P, c0, E, triples + 3 * q, side == 1, cand);
        float* out = scores + q * E;
        for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) out[e] = qv + cand[e];
    }
}

// one wave per sweep (2 n of them): rank = #{e : s_e < s_true}, filtered rank = rank - #{known e != true : s_e < s_true}
__global__ __launch_bounds__(kBlock) void k_convkb_ranks(const float* __restrict__ P, const float* __restrict__ A, int k, int64_t E,
                                                         const int64_t* __restrict__ triples, int64_t n,
                                                         const int64_t* __restrict__ tail_off, const int32_t* __restrict__ tail_ids,
                                                         const int64_t* __restrict__ head_off, const int32_t* __restrict__ head_ids,
                                                         int32_t* __restrict__ ranks) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= 2 * n) return;
    const int64_t i = q >> 1;
    const bool head = (q & 1) != 0;
    const float* cand;
    const float qv = ckb_query(P, A[3 * k], E, triples + 3 * i, head, cand);
    const int64_t tr = triples[3 * i + (head ? 0 : 2)];
    const float st = qv + cand[tr];
    int cnt = 0, fc = 0;
    for (int64_t e = lane; e < E; e += 64) cnt += (qv + cand[e]) < st ? 1 : 0;
    const int64_t* off = head ? head_off : tail_off;
    const int32_t* ids = head ? head_ids : tail_ids;
    if (off) {
        for (int64_t j = off[i] + lane; j < off[i + 1]; j += 64) {
            const int64_t e = ids[j];
            fc += (e != tr && (qv + cand[e]) < st) ? 1 : 0;
        }
    }
    cnt = (int)wave_sum((float)cnt);
    fc = (int)wave_sum((float)fc);
    if (lane == 0) {
        ranks[(head ? 0 : 1) * n + i] = cnt;
        ranks[(head ? 2 : 3) * n + i] = cnt - fc;
    }
}

// ---------------------------------------------------------------- host side
static int ckb_group(int k) { return k <= 256 ? 32 : 64; }   // the lane group: also the most rows a bundle may hold

static int ckb_check(const kge_convkb_desc* d, const char* who, bool grads) {
    if (!d) { set_error("%s: null descriptor", who); return -1; }
    if (!d->ent || !d->rel || !d->fc_w || !d->fc_b || !d->conv_w || !d->conv_b) {
        set_error("%s: null tables (ent, rel, fc_w, fc_b, conv_w and conv_b are all required)", who);
        return -1;
    }
    if (d->tot_entity < 1 || d->tot_relation < 1 || d->dim < 1) {
        set_error("%s: tot_entity, tot_relation and dim must be positive (got %lld, %lld, %d)", who, (long long)d->tot_entity,
                  (long long)d->tot_relation, d->dim);
        return -1;
    }
    if (d->num_filters < 1) { set_error("%s: num_filters must be at least 1 (got %d)", who, d->num_filters); return -1; }
    if (d->n_widths < 1 || d->n_widths > KGE_CONVKB_MAX_WIDTHS) {
        set_error("%s: n_widths must be 1..%d (got %d)", who, KGE_CONVKB_MAX_WIDTHS, d->n_widths);
        return -1;
    }
    int64_t W = 0;
    for (int j = 0; j < d->n_widths; ++j) {
        if (d->widths[j] < 1 || d->widths[j] > d->dim) {
            set_error("%s: filter width %d (position %d) outside 1..dim = %d", who, d->widths[j], j, d->dim);
            return -1;
        }
        W += d->dim - d->widths[j] + 1;
    }
    if ((int64_t)d->num_filters * W >= (int64_t(1) << 31)) { set_error("%s: fc1 has more than 2^31 inputs", who); return -1; }
    if (grads && (!d->g_ent || !d->g_rel || !d->g_fc_w || !d->g_fc_b)) {
        set_error("%s: null gradient buffers (g_ent, g_rel, g_fc_w and g_fc_b are all required)", who);
        return -1;
    }
    return 0;
}

static CkbGeom ckb_geom(const kge_convkb_desc* d) {
    CkbGeom g{};
    g.k = d->dim; g.F = d->num_filters; g.nw = d->n_widths;
    int off = 0, woff = 0;
    for (int j = 0; j < g.nw; ++j) {
        g.s[j] = d->widths[j]; g.off[j] = off; g.woff[j] = woff;
        off += g.k - g.s[j] + 1;
        woff += g.F * 3 * g.s[j];
    }
    g.W = off;
    return g;
}

static size_t ckb_vec_bytes(const kge_convkb_desc* d) { return align256((size_t)(3 * (int64_t)d->dim + 1) * sizeof(float)); }
static int ckb_slices(int k, int64_t n_bundles) {
    const int gpb = kBlock / ckb_group(k);
    int64_t blocks = (n_bundles + gpb - 1) / gpb;
    if (blocks > kCkbMaxSlices / gpb) blocks = kCkbMaxSlices / gpb;
    if (blocks < 1) blocks = 1;
    return (int)blocks * gpb;
}
// workspace of the step / backward: A | X | part (sized for single-row bundles, the most groups a call on n rows can launch)
static size_t ckb_step_bytes(const kge_convkb_desc* d, int64_t n) {
    const size_t vec = ckb_vec_bytes(d);
    return 2 * vec + align256((size_t)ckb_slices(d->dim, n) * (size_t)(3 * (int64_t)d->dim + 1) * sizeof(float));
}
static size_t ckb_eval_bytes(const kge_convkb_desc* d) {
    return ckb_vec_bytes(d) + align256((size_t)(2 * d->tot_entity + d->tot_relation) * sizeof(float));
}

static int ckb_collapse(const kge_convkb_desc* d, float* out, hipStream_t s) {
    const CkbGeom g = ckb_geom(d);
    const unsigned blocks = (unsigned)((3 * g.k + kBlock - 1) / kBlock) + 1;
    hipLaunchKernelGGL(k_convkb_collapse, dim3(blocks), dim3(kBlock), 0, s, g, d->conv_w, d->conv_b, d->fc_w, d->fc_b, out);
    return check_launch("k_convkb_collapse");
}

static CkbArgs ckb_args(const kge_convkb_desc* d, const float* A, float* part) {
    return CkbArgs{d->ent, d->rel, d->g_ent, d->g_rel, A, part, d->dim};
}

// collapse -> step -> finish -> fc1 gradient, on one stream
static int ckb_step(const kge_convkb_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, const int64_t* y,
                    const float* dscore, int64_t n, int bundle, void* ws, float* loss, const FusedSampler& fs, hipStream_t s) {
    const size_t vec = ckb_vec_bytes(d);
    float* A = (float*)ws;
    float* X = (float*)((char*)ws + vec);
    float* part = (float*)((char*)ws + 2 * vec);
    if (int rc = ckb_collapse(d, A, s)) return rc;
    const int G = ckb_group(d->dim);
    const int slices = ckb_slices(d->dim, (n + bundle - 1) / bundle);
    const CkbArgs a = ckb_args(d, A, part);
    const dim3 grid((unsigned)(slices / (kBlock / G))), block(kBlock);
    if (fs.triples) {
        if (G == 32) hipLaunchKernelGGL((k_convkb_step<32, true>), grid, block, 0, s, a, h, r, t, y, dscore, n, bundle, loss, fs);
        else hipLaunchKernelGGL((k_convkb_step<64, true>), grid, block, 0, s, a, h, r, t, y, dscore, n, bundle, loss, fs);
    } else {
        if (G == 32) hipLaunchKernelGGL((k_convkb_step<32, false>), grid, block, 0, s, a, h, r, t, y, dscore, n, bundle, loss, fs);
        else hipLaunchKernelGGL((k_convkb_step<64, false>), grid, block, 0, s, a, h, r, t, y, dscore, n, bundle, loss, fs);
    }
    if (int rc = check_launch("k_convkb_step")) return rc;
    const int width = 3 * d->dim + 1;
    hipLaunchKernelGGL(k_convkb_finish, dim3((unsigned)((width + 63) / 64)), dim3(64 * kCkbFinishWaves), 0, s, part, slices, width, X);
    const CkbGeom g = ckb_geom(d);
    hipLaunchKernelGGL(k_convkb_fc_grad, dim3((unsigned)((g.F * g.W + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, g, d->conv_w, d->conv_b,
                       X, d->g_fc_w, d->g_fc_b);
    return check_launch("k_convkb_finish / k_convkb_fc_grad");
}

static kge_model_desc ckb_id_bounds(const kge_convkb_desc* d) {   // what the id scans of the debug mode read
    kge_model_desc m{};
    m.tot_entity = d->tot_entity; m.tot_relation = d->tot_relation;
    return m;
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_convkb_collapse_workspace_bytes(const kge_convkb_desc* d) { (void)d; return 0; }

int kge_convkb_collapse(const kge_convkb_desc* d, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    if (ckb_check(d, "kge_convkb_collapse", false)) return -1;
    if (!out) { set_error("kge_convkb_collapse: bad arguments (out is null)"); return -1; }
    return ckb_collapse(d, out, (hipStream_t)stream);
}

size_t kge_convkb_score_forward_workspace_bytes(const kge_convkb_desc* d, int64_t n) {
    (void)n;
    return ckb_check(d, "kge_convkb_score_forward_workspace_bytes", false) ? 0 : ckb_vec_bytes(d);
}

int kge_convkb_score_forward(const kge_convkb_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n, float* scores,
                             void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_convkb_score_forward";
    if (ckb_check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!h || !r || !t || !scores))) { set_error("%s: bad arguments", who); return -1; }
    if (ws_check(who, workspace, workspace_bytes, ckb_vec_bytes(d))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const kge_model_desc bounds = ckb_id_bounds(d);
    if (int rc = debug_check_hrt(who, &bounds, h, r, t, n, s)) return rc;
    if (int rc = ckb_collapse(d, (float*)workspace, s)) return rc;
    const int G = ckb_group(d->dim);
    const CkbArgs a = ckb_args(d, (const float*)workspace, nullptr);
    int64_t blocks = (n + kBlock / G - 1) / (kBlock / G);
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    if (G == 32) hipLaunchKernelGGL((k_convkb_forward<32>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a, h, r, t, n, scores);
    else hipLaunchKernelGGL((k_convkb_forward<64>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a, h, r, t, n, scores);
    return check_launch("k_convkb_forward");
}

size_t kge_convkb_score_backward_workspace_bytes(const kge_convkb_desc* d, int64_t n) {
    return ckb_check(d, "kge_convkb_score_backward_workspace_bytes", false) || n < 0 ? 0 : ckb_step_bytes(d, n);
}

int kge_convkb_score_backward(const kge_convkb_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n,
                              const float* dscore, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_convkb_score_backward";
    if (ckb_check(d, who, true)) return -1;
    if (n < 0 || (n > 0 && (!h || !r || !t || !dscore))) { set_error("%s: bad arguments", who); return -1; }
    if (ws_check(who, workspace, workspace_bytes, ckb_step_bytes(d, n))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const kge_model_desc bounds = ckb_id_bounds(d);
    if (int rc = debug_check_hrt(who, &bounds, h, r, t, n, s)) return rc;
    return ckb_step(d, h, r, t, nullptr, dscore, n, 1, workspace, nullptr, FusedSampler{}, s);
}

size_t kge_convkb_train_logistic_workspace_bytes(const kge_convkb_desc* d, int64_t n) {
    return ckb_check(d, "kge_convkb_train_logistic_workspace_bytes", false) || n < 0 ? 0 : ckb_step_bytes(d, n);
}

int kge_convkb_train_logistic(const kge_convkb_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, const int64_t* y,
                              int64_t n, int32_t bundle, void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    const char* who = "kge_convkb_train_logistic";
    if (ckb_check(d, who, true)) return -1;
    if (n < 0 || !loss || (n > 0 && (!h || !r || !t || !y))) { set_error("%s: bad arguments", who); return -1; }
    if (ws_check(who, workspace, workspace_bytes, ckb_step_bytes(d, n))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const kge_model_desc bounds = ckb_id_bounds(d);
    if (int rc = debug_check_hrt(who, &bounds, h, r, t, n, s)) return rc;
    // a member's coefficient waits in lane m of the group between the passes: longer bundles run row by row (exact either way)
    if (bundle < 1 || bundle > ckb_group(d->dim)) bundle = 1;
    return ckb_step(d, h, r, t, y, nullptr, n, bundle, workspace, loss, FusedSampler{}, s);
}

size_t kge_convkb_train_logistic_sampled_workspace_bytes(const kge_convkb_desc* d, int64_t n_pos, int32_t neg_rate) {
    (void)neg_rate;
    return ckb_check(d, "kge_convkb_train_logistic_sampled_workspace_bytes", false) || n_pos < 0 ? 0 : ckb_step_bytes(d, n_pos);
}

int kge_convkb_train_logistic_sampled(const kge_convkb_desc* d, const int64_t* triples, const int64_t* perm, int64_t start,
                                      int64_t n_pos, int32_t neg_rate, const float* bern_prob, const uint64_t* slots,
                                      int64_t n_slots, uint64_t seed, uint64_t offset, const int64_t* dev_cursor, void* workspace,
                                      size_t workspace_bytes, float* loss, void* stream) {
    const char* who = "kge_convkb_train_logistic_sampled";
    if (ckb_check(d, who, true)) return -1;
    if (n_pos < 0 || neg_rate < 1 || start < 0 || !loss || (n_pos > 0 && (!triples || !perm))) { set_error("%s: bad arguments", who); return -1; }
    if (slots && (n_slots & (n_slots - 1))) { set_error("%s: n_slots must be a power of two", who); return -1; }
    if (d->tot_entity > (int64_t(1) << 24) || d->tot_relation > (int64_t(1) << 16)) {
        set_error("%s: the sampler's packed triple key takes at most 2^24 entities and 2^16 relations", who);
        return -1;
    }
    // the bundle's positive sits in lane 0 and negative j's draw in lane j, so 1 + neg_rate rows must fit one lane group
    if (1 + neg_rate > ckb_group(d->dim)) {
        set_error("%s: ConvKB with hidden size %d takes neg_rate <= %d", who, d->dim, ckb_group(d->dim) - 1);
        return -1;
    }
    if (ws_check(who, workspace, workspace_bytes, ckb_step_bytes(d, n_pos))) return -1;
    if (n_pos == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (!dev_cursor)
        if (int rc = debug_check_triples(who, d->tot_entity, d->tot_relation, triples, n_pos, s, perm, start)) return rc;
    FusedSampler fs;
    fs.triples = triples; fs.perm = perm; fs.start = start; fs.E = d->tot_entity; fs.bern = bern_prob;
    fs.slots = (const unsigned long long*)slots; fs.mask = (unsigned long long)(slots ? n_slots - 1 : 0);
    fs.seed = seed; fs.offset = offset; fs.cursor = dev_cursor;
    return ckb_step(d, nullptr, nullptr, nullptr, nullptr, nullptr, n_pos * (1 + (int64_t)neg_rate), 1 + neg_rate, workspace, loss, fs, s);
}

size_t kge_convkb_eval_ranks_workspace_bytes(const kge_convkb_desc* d, int64_t n) {
    (void)n;
    return ckb_check(d, "kge_convkb_eval_ranks_workspace_bytes", false) ? 0 : ckb_eval_bytes(d);
}

size_t kge_convkb_sweep_scores_side_workspace_bytes(const kge_convkb_desc* d, int64_t n) {
    (void)n;
    return ckb_check(d, "kge_convkb_sweep_scores_side_workspace_bytes", false) ? 0 : ckb_eval_bytes(d);
}

// A and the projections P into the workspace
static int ckb_prepare_eval(const kge_convkb_desc* d, void* ws, hipStream_t s, const float** A, const float** P) {
    float* a = (float*)ws;
    float* p = (float*)((char*)ws + ckb_vec_bytes(d));
    if (int rc = ckb_collapse(d, a, s)) return rc;
    const int G = ckb_group(d->dim);
    const int64_t rows = d->tot_entity + d->tot_relation;
    int64_t blocks = (rows + kBlock / G - 1) / (kBlock / G);
    if (blocks > 4 * kMaxBlocks) blocks = 4 * kMaxBlocks;
    const CkbArgs args = ckb_args(d, a, nullptr);
    if (G == 32) hipLaunchKernelGGL((k_convkb_project<32>), dim3((unsigned)blocks), dim3(kBlock), 0, s, args, d->tot_entity, d->tot_relation, p);
    else hipLaunchKernelGGL((k_convkb_project<64>), dim3((unsigned)blocks), dim3(kBlock), 0, s, args, d->tot_entity, d->tot_relation, p);
    *A = a; *P = p;
    return check_launch("k_convkb_project");
}

int kge_convkb_eval_ranks(const kge_convkb_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                          const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks,
                          void* stream) {
    const char* who = "kge_convkb_eval_ranks";
    if (ckb_check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!triples || !ranks)) || (tail_off && !tail_ids) || (head_off && !head_ids)) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    if (ws_check(who, workspace, workspace_bytes, ckb_eval_bytes(d))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = debug_check_triples(who, d->tot_entity, d->tot_relation, triples, n, s)) return rc;
    const float *A, *P;
    if (int rc = ckb_prepare_eval(d, workspace, s, &A, &P)) return rc;
    hipLaunchKernelGGL(k_convkb_ranks, dim3((unsigned)((2 * n + 3) / 4)), dim3(kBlock), 0, s, P, A, d->dim, d->tot_entity, triples, n,
                       tail_off, tail_ids, head_off, head_ids, ranks);
    return check_launch("k_convkb_ranks");
}

int kge_convkb_sweep_scores_side(const kge_convkb_desc* d, const int64_t* triples, int64_t n, int side, void* workspace,
                                 size_t workspace_bytes, float* scores, void* stream) {
    const char* who = "kge_convkb_sweep_scores_side";
    if (ckb_check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!triples || !scores)) || (side != 0 && side != 1)) {
        set_error("%s: bad arguments (side is 0 = tail sweep or 1 = head sweep)", who);
        return -1;
    }
    if (ws_check(who, workspace, workspace_bytes, ckb_eval_bytes(d))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = debug_check_triples(who, d->tot_entity, d->tot_relation, triples, n, s)) return rc;
    const float *A, *P;
    if (int rc = ckb_prepare_eval(d, workspace, s, &A, &P)) return rc;
    const int64_t E = d->tot_entity;
    const unsigned bx = (unsigned)((E + kBlock - 1) / kBlock > 64 ? 64 : (E + kBlock - 1) / kBlock);
    const unsigned by = (unsigned)(n > 4096 ? 4096 : n);
    hipLaunchKernelGGL(k_convkb_sweep, dim3(bx, by), dim3(kBlock), 0, s, P, A, d->dim, E, triples, n, side, scores);
    return check_launch("k_convkb_sweep");
}

}  // extern "C"
