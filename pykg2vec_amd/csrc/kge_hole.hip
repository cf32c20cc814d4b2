// kge_hole.hip -- HoLE (pairwise.py:1087-1142): forward, backward, the pairwise hinge step's two halves and the rank sweep.
//
// The reference runs on torch < 1.7, where torch.fft(x, 1) maps real [..., d, 2] tensors to real [..., d, 2] tensors, torch.conj
// is the identity on them and `*` multiplies real with real and imaginary with imaginary parts.  With C[j,k] = cos(2 pi jk/d)
// and S[j,k] = sin(2 pi jk/d) (both symmetric) the model as it shipped computes
//     x = (1/d) sum_j [ (C h)_j (C t)_j (C r^)_j - (S h)_j (S t)_j (S r^)_j ],   energy = -sigmoid(x),   r^ = F.normalize(r)
// (DESIGN.md section 9).  This file evaluates that form directly on the VALU: one wave per triple, the three gathered rows and
// their six projections in LDS, the basis generated per workgroup as a table of d angles cos / sin(2 pi p / d) (double
// precision, p = (j k) mod d walked incrementally, so the angle stays exact at any d).  O(d^2) per triple: 6 d^2 FMAs forward,
// as many again backward -- at the FB15k preset (d = 150) about 0.3 GFLOP per step.
//
//   forward / pair forward   energies of [positives | negatives] (IdSplit), one launch
//   backward / pair backward recompute the projections, back-project with [C | S]^T, normalisation backward of r,
//                            float-atomic scatter of the h, t and r rows (summation order varies run to run: DESIGN.md section 9)
//   rank                     candidate rows [C e | S e] (K = 2d), query rows (1/d) [(C q)(C r^) | -(S q)(S r^)] with q = h for the
//                            tail sweep and q = t for the head sweep (x is symmetric in h and t); the negated-dot pipeline of
//                            kge_eval.hip with its sigmoid post-op returns -sigmoid(x), so ranks see the reference's fp32 ties.
#include "kge_internal.h"

namespace kge {

constexpr int kHoleMaxDim = 2048;

static int hole_waves(int d) { return d <= 256 ? 4 : 1; }
// LDS floats: angle tables (2d) + per wave rows h, t, r^ (3d) and projections Ch, Sh, Ct, St, Cr, Sr (6d)
static size_t hole_lds(int d) { return (size_t)(2 * d + 9 * d * hole_waves(d)) * sizeof(float); }

static int hole_check(const kge_model_desc* m, const char* who) {
    if (m->model != KGE_HOLE) { set_error("%s: not a HoLE descriptor (model %d)", who, m->model); return -1; }
    if (m->dim > kHoleMaxDim) { set_error("%s: HoLE takes hidden sizes 1..%d (got %d)", who, kHoleMaxDim, m->dim); return -1; }
    return 0;
}

__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// cs[p] = cos(2 pi p / d), sn[p] = sin(2 pi p / d), p < d; the whole block, followed by a block barrier
__device__ __forceinline__ void hole_angles(float* cs, float* sn, int d) {
    for (int p = threadIdx.x; p < d; p += blockDim.x) {
        double s, c;
        sincospi(2.0 * (double)p / (double)d, &s, &c);
        cs[p] = (float)c; sn[p] = (float)s;
    }
    __syncthreads();
}

// (C x)_j and (S x)_j for the three LDS rows x = a, b, c: row j of C / S walks the angle index (j k) mod d
__device__ __forceinline__ void hole_project3(const float* cs, const float* sn, int d, int j, const float* a, const float* b,
                                              const float* c, float (&o)[6]) {
    float ca = 0.f, sa = 0.f, cb = 0.f, sb = 0.f, cc = 0.f, sc = 0.f;
    int p = 0;
    for (int k = 0; k < d; ++k) {
        const float co = cs[p], si = sn[p];
        ca = fmaf(co, a[k], ca); sa = fmaf(si, a[k], sa);
        cb = fmaf(co, b[k], cb); sb = fmaf(si, b[k], sb);
        cc = fmaf(co, c[k], cc); sc = fmaf(si, c[k], sc);
        p += j;
        if (p >= d) p -= d;
    }
    o[0] = ca; o[1] = sa; o[2] = cb; o[3] = sb; o[4] = cc; o[5] = sc;
}

struct HoleArgs {
    const float* ent; const float* rel; float* gent; float* grel;
    IdSplit h, r, t;
    int64_t n;
    int d;
};

// BWD = false: scores[i] = energy.  BWD = true: scatter d(dscore[i] * energy) into gent / grel.
template <bool BWD>
__global__ __launch_bounds__(256) void k_hole(HoleArgs a, float* __restrict__ scores, const float* __restrict__ dscore) {
    extern __shared__ float smem[];
    const int d = a.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
    float* cs = smem;
    float* sn = cs + d;
    float* xh = sn + d + wave * 9 * d;
    float* xt = xh + d;
    float* xr = xt + d;
    float* pj = xr + d;   // [6][d]: Ch, Sh, Ct, St, Cr, Sr
    hole_angles(cs, sn, d);
    const float invd = 1.0f / (float)d;
    for (int64_t i = (int64_t)blockIdx.x * W + wave; i < a.n; i += (int64_t)gridDim.x * W) {
        float ds = 0.f;
        if constexpr (BWD) {
            ds = dscore[i];
            if (ds == 0.f) continue;   // wave-uniform
        }
        const int64_t h = a.h.at(i), r = a.r.at(i), t = a.t.at(i);
        const float* eh = a.ent + h * d; const float* et = a.ent + t * d; const float* er = a.rel + r * d;
        float nr = 0.f;
        for (int k = lane; k < d; k += 64) {
            const float v = er[k];
            xh[k] = eh[k]; xt[k] = et[k]; xr[k] = v;
            nr = fmaf(v, v, nr);
        }
        const float rn = sqrtf(wave_sum(nr));
        const float ir = 1.0f / fmaxf(rn, kEpsNormalize);
        for (int k = lane; k < d; k += 64) xr[k] *= ir;
        wave_sync_lds();
        float part = 0.f;
        for (int j = lane; j < d; j += 64) {
            float o[6];
            hole_project3(cs, sn, d, j, xh, xt, xr, o);
            part += o[0] * o[2] * o[4] - o[1] * o[3] * o[5];
            if constexpr (BWD) {
#pragma unroll
                for (int q = 0; q < 6; ++q) pj[q * d + j] = o[q];
            }
        }
        const float x = wave_sum(part) * invd;
        const float sg = 1.0f / (1.0f + expf(-x));
        if constexpr (!BWD) {
            if (lane == 0) scores[i] = -sg;
        } else {
            wave_sync_lds();
            const float g = -ds * sg * (1.0f - sg) * invd;   // d(ds * energy) / d(sum_j ...)
            const float *Ch = pj, *Sh = pj + d, *Ct = pj + 2 * d, *St = pj + 3 * d, *Cr = pj + 4 * d, *Sr = pj + 5 * d;
            // C and S are symmetric: column k of the back-projection walks the same angle index as row k.  The h and t rows scatter
            // at once; d/d r^ waits in xh (no longer read) for the normalisation backward's dot product.
            float dot = 0.f;
            for (int k = lane; k < d; k += 64) {
                float ah = 0.f, at = 0.f, ar = 0.f;
                int p = 0;
                for (int jj = 0; jj < d; ++jj) {
                    const float co = cs[p], si = sn[p];
                    ah += co * (Ct[jj] * Cr[jj]) - si * (St[jj] * Sr[jj]);
                    at += co * (Ch[jj] * Cr[jj]) - si * (Sh[jj] * Sr[jj]);
                    ar += co * (Ch[jj] * Ct[jj]) - si * (Sh[jj] * St[jj]);
                    p += k;
                    if (p >= d) p -= d;
                }
                unsafeAtomicAdd(a.gent + h * d + k, g * ah);
                unsafeAtomicAdd(a.gent + t * d + k, g * at);
                xh[k] = g * ar;
                dot = fmaf(xr[k], g * ar, dot);
            }
            dot = wave_sum(dot);
            for (int k = lane; k < d; k += 64) {
                // F.normalize backward: (g - r^ (r^ . g)) / |r| above eps, g / eps below
                const float gr = xh[k];
                unsafeAtomicAdd(a.grel + r * d + k, rn > kEpsNormalize ? (gr - xr[k] * dot) * ir : gr * ir);
            }
        }
        wave_sync_lds();   // the next triple overwrites this wave's rows
    }
}

static void hole_lds_attr() {
    static const bool done = [] {
        const int most = (int)hole_lds(kHoleMaxDim);
        bool ok = hipFuncSetAttribute((const void*)k_hole<false>, hipFuncAttributeMaxDynamicSharedMemorySize, most) == hipSuccess;
        ok = hipFuncSetAttribute((const void*)k_hole<true>, hipFuncAttributeMaxDynamicSharedMemorySize, most) == hipSuccess && ok;
        return ok;
    }();
    (void)done;
}

static int hole_run(const kge_model_desc* m, IdSplit h, IdSplit r, IdSplit t, int64_t N, float* scores, const float* dscore,
                    hipStream_t s) {
    if (hole_check(m, dscore ? "kge_score_backward" : "kge_score_forward")) return -1;
    if (N <= 0) return 0;
    hole_lds_attr();
    const int d = m->dim, W = hole_waves(d);
    int64_t blocks = (N + W - 1) / W;
    if (blocks > 2048) blocks = 2048;
    HoleArgs a{m->tables[0], m->tables[1], m->grads[0], m->grads[1], h, r, t, N, d};
    if (dscore) {
        hipLaunchKernelGGL(k_hole<true>, dim3((unsigned)blocks), dim3(64 * W), hole_lds(d), s, a, nullptr, dscore);
        return check_launch("k_hole<backward>");
    }
    hipLaunchKernelGGL(k_hole<false>, dim3((unsigned)blocks), dim3(64 * W), hole_lds(d), s, a, scores, nullptr);
    return check_launch("k_hole<forward>");
}

// (table signatures: HoLE needs no scorer workspace and ignores the one it is handed)
int launch_hole_forward(const kge_model_desc* m, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n, float* scores,
                        void*, size_t, hipStream_t s) {
    return hole_run(m, id_whole(h, n), id_whole(r, n), id_whole(t, n), n, scores, nullptr, s);
}

int launch_hole_backward(const kge_model_desc* m, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n,
                         const float* dscore, void*, size_t, hipStream_t s) {
    return hole_run(m, id_whole(h, n), id_whole(r, n), id_whole(t, n), n, nullptr, dscore, s);
}

int launch_hole_pair_forward(const kge_model_desc* m, const int64_t* ph, const int64_t* pr, const int64_t* pt, const int64_t* nh,
                             const int64_t* nr, const int64_t* nt, int64_t n, float* scores2, void*, size_t, hipStream_t s) {
    return hole_run(m, IdSplit{ph, nh, n}, IdSplit{pr, nr, n}, IdSplit{pt, nt, n}, 2 * n, scores2, nullptr, s);
}

int launch_hole_pair_backward(const kge_model_desc* m, const int64_t* ph, const int64_t* pr, const int64_t* pt, const int64_t* nh,
                              const int64_t* nr, const int64_t* nt, int64_t n, const float* dscore2, void*, size_t, hipStream_t s) {
    return hole_run(m, IdSplit{ph, nh, n}, IdSplit{pr, nr, n}, IdSplit{pt, nt, n}, 2 * n, nullptr, dscore2, s);
}

// ---------------------------------------------------------------- rank: candidate rows [C e | S e], query rows, the dot pipeline
// one wave per entity; LDS: angle tables + 4 rows
__global__ __launch_bounds__(256) void k_hole_cand(const float* __restrict__ ent, int64_t E, int d, float* __restrict__ cand) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* cs = smem;
    float* sn = cs + d;
    float* x = sn + d + wave * d;
    hole_angles(cs, sn, d);
    const int64_t e = (int64_t)blockIdx.x * 4 + wave;
    if (e >= E) return;
    for (int k = lane; k < d; k += 64) x[k] = ent[e * d + k];
    wave_sync_lds();
    float* o = cand + e * (int64_t)(2 * d);
    for (int j = lane; j < d; j += 64) {
        float c = 0.f, s = 0.f;
        int p = 0;
        for (int k = 0; k < d; ++k) {
            c = fmaf(cs[p], x[k], c); s = fmaf(sn[p], x[k], s);
            p += j;
            if (p >= d) p -= d;
        }
        o[j] = c; o[d + j] = s;
    }
}

// one wave per test triple: rows 2i (tail sweep, q = h) and 2i + 1 (head sweep, q = t) of width 2d
__global__ __launch_bounds__(256) void k_hole_queries(const float* __restrict__ ent, const float* __restrict__ rel,
                                                      const int64_t* __restrict__ triples, int64_t n, int d, float* __restrict__ qrows) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* cs = smem;
    float* sn = cs + d;
    float* xh = sn + d + wave * 3 * d;
    float* xt = xh + d;
    float* xr = xt + d;
    hole_angles(cs, sn, d);
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= n) return;
    const int64_t h = triples[3 * i], r = triples[3 * i + 1], t = triples[3 * i + 2];
    float nr = 0.f;
    for (int k = lane; k < d; k += 64) {
        const float v = rel[r * d + k];
        xh[k] = ent[h * d + k]; xt[k] = ent[t * d + k]; xr[k] = v;
        nr = fmaf(v, v, nr);
    }
    const float ir = 1.0f / fmaxf(sqrtf(wave_sum(nr)), kEpsNormalize);
    for (int k = lane; k < d; k += 64) xr[k] *= ir;
    wave_sync_lds();
    const float invd = 1.0f / (float)d;
    float* qt = qrows + 2 * i * (int64_t)(2 * d);
    float* qh = qt + 2 * d;
    for (int j = lane; j < d; j += 64) {
        float o[6];
        hole_project3(cs, sn, d, j, xh, xt, xr, o);
        qt[j] = (o[0] * o[4]) * invd; qt[d + j] = -(o[1] * o[5]) * invd;
        qh[j] = (o[2] * o[4]) * invd; qh[d + j] = -(o[3] * o[5]) * invd;
    }
}

size_t hole_eval_workspace_bytes(const kge_model_desc* m, int64_t n) {
    return dot_rows_plan(nullptr, m->tot_entity, n, 2 * m->dim, true).bytes;
}

static void hole_eval_lds_attr() {
    static const bool done = [] {
        const int most = (int)((size_t)(2 + 4 * 3) * kHoleMaxDim * sizeof(float));
        bool ok = hipFuncSetAttribute((const void*)k_hole_cand, hipFuncAttributeMaxDynamicSharedMemorySize, most) == hipSuccess;
        ok = hipFuncSetAttribute((const void*)k_hole_queries, hipFuncAttributeMaxDynamicSharedMemorySize, most) == hipSuccess && ok;
        return ok;
    }();
    (void)done;
}

int launch_hole_eval(const kge_model_desc* m, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                     const int64_t* head_off, const int32_t* head_ids, void* ws, size_t ws_bytes, int32_t* ranks, int32_t* ties,
                     float* scores, hipStream_t s, int side) {
    if (hole_check(m, "kge_eval")) return -1;
    const DotRowsPlan w = dot_rows_plan(ws, m->tot_entity, n, 2 * m->dim, true);
    if (!ws || ws_bytes < w.bytes) { set_error("kge_eval (HoLE): workspace too small (%zu < %zu)", ws_bytes, w.bytes); return -1; }
    if (n <= 0) return 0;
    hole_eval_lds_attr();
    const int64_t E = m->tot_entity;
    const int d = m->dim;
    hipLaunchKernelGGL(k_hole_cand, dim3((unsigned)((E + 3) / 4)), dim3(256), (size_t)(2 + 4) * d * sizeof(float), s, m->tables[0], E,
                       d, w.cand);
    hipLaunchKernelGGL(k_hole_queries, dim3((unsigned)((n + 3) / 4)), dim3(256), (size_t)(2 + 4 * 3) * d * sizeof(float), s,
                       m->tables[0], m->tables[1], triples, n, d, w.qrows);
    if (int rc = check_launch("k_hole_cand / k_hole_queries")) return rc;
    return launch_dot_eval(w.cand, w.qrows, 2 * d, E, triples, n, tail_off, tail_ids, head_off, head_ids, w.pipe, w.pipe_bytes,
                           ranks, ties, scores, s, side, true);
}

}  // namespace kge
