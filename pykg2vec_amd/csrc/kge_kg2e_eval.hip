// kge_kg2e_eval.hip -- filtered rank for KG2E (pairwise.py:966-1084) as an elementwise VALU sweep.
//
// energy(h, r, t) = sum cs/t^s + sum (t^m - cm)^2 / t^s + sum (log t^s - log cs) - d,  cs = h^s + r^s, cm = h^m + r^m,
// every row divided by its own L2 norm (no eps).  Per evaluation the candidate side is prepared once: normalised mu and sigma
// rows stored k-major (cmu[k E + e], csg[k E + e]: thread = candidate, coalesced) and clog[e] = sum_k log(e^s_k).
//   tail sweep (h, r, ?):  query A = cm, B = cs, constant -sum log cs; per element  B/ts + (tm - A)^2/ts, plus clog[e]
//   head sweep (?, r, t):  query A = r^m, B = r^s, C = t^m, D = t^s, constant sum log t^s; per element cs = hs + B,
//                          cs/D + (C - (hm + A))^2/D and one log(cs) -- h^s + r^s does not separate
// The per-element order differs from the reference's three sums; energies agree with kge_score_forward to fp32 rounding.  Queries
// run in chunks whose energies are materialised ([rows, E] fp32) and ranked from those very values (count + CSR filter + ties),
// so ranks are exact functions of the returned energies.
#include "kge_internal.h"

namespace kge {

constexpr int kKg2eMaxDim = 2048;
constexpr int kKg2eChunk = 256;   // test triples per scored chunk

struct Kg2eEvalWs {
    float *cmu, *csg, *clog, *q4, *qc, *scores;
    int64_t* truth;
    int chunk;
    size_t bytes;
};

static void kg2e_eval_plan(const kge_model_desc* m, int64_t n, void* ws, Kg2eEvalWs* w, int ns) {
    size_t off = 0;
    char* base = (char*)ws;
    auto take = [&](size_t b) { char* p = base ? base + off : nullptr; off += align256(b); return p; };
    const int64_t E = m->tot_entity;
    const int d = m->dim;
    w->chunk = (int)(n < kKg2eChunk ? (n < 1 ? 1 : n) : kKg2eChunk);
    const int64_t Q = (int64_t)ns * w->chunk;   // query rows per chunk
    w->cmu = (float*)take((size_t)d * E * 4);
    w->csg = (float*)take((size_t)d * E * 4);
    w->clog = (float*)take((size_t)E * 4);
    w->q4 = (float*)take((size_t)Q * 4 * d * 4);
    w->qc = (float*)take((size_t)Q * 4);
    w->scores = (float*)take((size_t)Q * E * 4);
    w->truth = (int64_t*)take((size_t)Q * 8);
    w->bytes = off;
}

size_t kg2e_eval_workspace_bytes(const kge_model_desc* m, int64_t n) {
    Kg2eEvalWs w;
    kg2e_eval_plan(m, n, nullptr, &w, 2);
    return w.bytes;
}

// one wave per entity: normalised mu / sigma rows, k-major, and sum_k log(sigma^_k)
__global__ __launch_bounds__(256) void k_kg2e_cand(const float* __restrict__ mu, const float* __restrict__ sg, int64_t E, int d,
                                                   float* __restrict__ cmu, float* __restrict__ csg, float* __restrict__ clog) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    const float* xm = mu + e * d; const float* xs = sg + e * d;
    float nm = 0.f, ns = 0.f;
    for (int k = lane; k < d; k += 64) { nm = fmaf(xm[k], xm[k], nm); ns = fmaf(xs[k], xs[k], ns); }
    const float im = 1.0f / sqrtf(wave_sum(nm)), is = 1.0f / sqrtf(wave_sum(ns));
    float lg = 0.f;
    for (int k = lane; k < d; k += 64) {
        const float s = xs[k] * is;
        cmu[(int64_t)k * E + e] = xm[k] * im;
        csg[(int64_t)k * E + e] = s;
        lg += logf(s);
    }
    lg = wave_sum(lg);
    if (lane == 0) clog[e] = lg;
}

// one wave per query row q of the chunk: triple lo + q / ns, side = ns == 2 ? q & 1 : side (0 = tail sweep, 1 = head sweep)
__global__ __launch_bounds__(256) void k_kg2e_queries(const kge_model_desc md, const int64_t* __restrict__ triples, int64_t nq,
                                                      int ns, int side, Kg2eEvalWs w) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int d = md.dim;
    const int64_t i = q / ns;
    const int sd = ns == 2 ? (int)(q & 1) : side;
    const int64_t h = triples[3 * i], r = triples[3 * i + 1], t = triples[3 * i + 2];
    const float *ent_mu = md.tables[0], *ent_sg = md.tables[1], *rel_mu = md.tables[2], *rel_sg = md.tables[3];
    const float* rm = rel_mu + r * d; const float* rs = rel_sg + r * d;
    const float* em = ent_mu + (sd == 0 ? h : t) * d; const float* es = ent_sg + (sd == 0 ? h : t) * d;
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;
    for (int k = lane; k < d; k += 64) {
        n0 = fmaf(rm[k], rm[k], n0); n1 = fmaf(rs[k], rs[k], n1);
        n2 = fmaf(em[k], em[k], n2); n3 = fmaf(es[k], es[k], n3);
    }
    const float irm = 1.0f / sqrtf(wave_sum(n0)), irs = 1.0f / sqrtf(wave_sum(n1));
    const float iem = 1.0f / sqrtf(wave_sum(n2)), ies = 1.0f / sqrtf(wave_sum(n3));
    float* Q = w.q4 + q * 4 * (int64_t)d;
    float c = 0.f;
    for (int k = lane; k < d; k += 64) {
        const float a = rm[k] * irm, b = rs[k] * irs, x = em[k] * iem, y = es[k] * ies;
        if (sd == 0) {   // x, y = h^m, h^s
            const float cs = y + b;
            Q[k] = x + a; Q[d + k] = cs;
            c -= logf(cs);
        } else {         // x, y = t^m, t^s
            Q[k] = a; Q[d + k] = b; Q[2 * d + k] = x; Q[3 * d + k] = y;
            c += logf(y);
        }
    }
    c = wave_sum(c);
    if (lane == 0) { w.qc[q] = c; w.truth[q] = sd == 0 ? t : h; }
}

// energies of query row q (blockIdx.y) against 256 candidates per workgroup: thread = candidate, the query in LDS
__global__ __launch_bounds__(256) void k_kg2e_sweep(int64_t E, int d, int ns, int side, Kg2eEvalWs w, float* __restrict__ scores) {
    __shared__ float sq[4 * kKg2eMaxDim];
    const int64_t q = blockIdx.y;
    const int sd = ns == 2 ? (int)(q & 1) : side;
    const int nv = sd == 0 ? 2 : 4;
    for (int k = threadIdx.x; k < nv * d; k += 256) sq[k] = w.q4[q * 4 * (int64_t)d + k];
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float qc = w.qc[q];
    float acc = 0.f;
    if (sd == 0) {
        for (int k = 0; k < d; ++k) {
            const float ts = w.csg[(int64_t)k * E + e], u = w.cmu[(int64_t)k * E + e] - sq[k];
            acc += sq[d + k] / ts + (u * u) / ts;
        }
        scores[q * E + e] = (acc + (w.clog[e] + qc)) - (float)d;
    } else {
        float lg = 0.f;
        for (int k = 0; k < d; ++k) {
            const float cs = w.csg[(int64_t)k * E + e] + sq[d + k];
            const float u = sq[2 * d + k] - (w.cmu[(int64_t)k * E + e] + sq[k]);
            const float ts = sq[3 * d + k];
            acc += cs / ts + (u * u) / ts;
            lg += logf(cs);
        }
        scores[q * E + e] = (acc + (qc - lg)) - (float)d;
    }
}

// one wave per query row: rank = #{e : s_e < s_true}, filtered = rank - #{known e != true : s_e < s_true}, ties = #{e != true :
// s_e == s_true}.  ranks rows: head, tail, fhead, ftail ([4, n]) or rank, filtered ([2, n]) one-sided; ties [2, n] (head, tail) or [n]
__global__ __launch_bounds__(256) void k_kg2e_rank_rows(const float* __restrict__ scores, int64_t nq, int ns, int side, int64_t E,
                                                        const int64_t* __restrict__ truth, const int64_t* __restrict__ tail_off,
                                                        const int32_t* __restrict__ tail_ids, const int64_t* __restrict__ head_off,
                                                        const int32_t* __restrict__ head_ids, int64_t tri0, int64_t n_total,
                                                        int32_t* __restrict__ ranks, int32_t* __restrict__ ties) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int64_t i = q / ns;
    const int sd = ns == 2 ? (int)(q & 1) : side;
    const float* s = scores + q * E;
    const int64_t tr = truth[q];
    const float stv = s[tr];
    int cnt = 0, eq = 0, fc = 0;
    for (int64_t e = lane; e < E; e += 64) { cnt += s[e] < stv ? 1 : 0; eq += s[e] == stv ? 1 : 0; }
    const int64_t* off = sd == 0 ? tail_off : head_off;
    const int32_t* ids = sd == 0 ? tail_ids : head_ids;
    if (off)
        for (int64_t j = off[tri0 + i] + lane; j < off[tri0 + i + 1]; j += 64) {
            const int64_t e = ids[j];
            fc += (e != tr && s[e] < stv) ? 1 : 0;
        }
    cnt = (int)wave_sum((float)cnt);
    eq = (int)wave_sum((float)eq);
    fc = (int)wave_sum((float)fc);
    if (lane != 0) return;
    const int64_t g = tri0 + i;
    if (ns == 2) {
        ranks[(sd == 0 ? 1 : 0) * n_total + g] = cnt;
        ranks[(sd == 0 ? 3 : 2) * n_total + g] = cnt - fc;
        if (ties) ties[(sd == 0 ? 1 : 0) * n_total + g] = max(0, eq - 1);
    } else {
        ranks[g] = cnt;
        ranks[n_total + g] = cnt - fc;
        if (ties) ties[g] = max(0, eq - 1);
    }
}

int launch_kg2e_eval(const kge_model_desc* m, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                     const int64_t* head_off, const int32_t* head_ids, void* ws, size_t ws_bytes, int32_t* ranks, int32_t* ties,
                     float* scores_out, hipStream_t s, int side) {
    if (m->model != KGE_KG2E) { set_error("kge_eval: not a KG2E descriptor (model %d)", m->model); return -1; }
    if (m->dim > kKg2eMaxDim) { set_error("kge_eval: KG2E takes hidden sizes 1..%d (got %d)", kKg2eMaxDim, m->dim); return -1; }
    const int ns = side == 2 ? 2 : 1;
    Kg2eEvalWs w;
    kg2e_eval_plan(m, n, ws, &w, ns);   // one-sided sweeps use a prefix of the two-sided layout
    if (!ws || ws_bytes < w.bytes) { set_error("kge_eval (KG2E): workspace too small (%zu < %zu)", ws_bytes, w.bytes); return -1; }
    if (n <= 0) return 0;
    const int64_t E = m->tot_entity;
    const int d = m->dim;
    hipLaunchKernelGGL(k_kg2e_cand, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, s, m->tables[0], m->tables[1], E, d, w.cmu, w.csg,
                       w.clog);
    for (int64_t lo = 0; lo < n; lo += w.chunk) {
        const int64_t c = min((int64_t)w.chunk, n - lo);
        const int64_t nq = ns * c;
        hipLaunchKernelGGL(k_kg2e_queries, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, *m, triples + 3 * lo, nq, ns, side, w);
        float* sc = scores_out ? scores_out + ns * lo * E : w.scores;
        hipLaunchKernelGGL(k_kg2e_sweep, dim3((unsigned)((E + 255) / 256), (unsigned)nq), dim3(256), 0, s, E, d, ns, side, w, sc);
        if (ranks)
            hipLaunchKernelGGL(k_kg2e_rank_rows, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, sc, nq, ns, side, E, w.truth,
                               tail_off, tail_ids, head_off, head_ids, lo, n, ranks, ties);
    }
    return check_launch("KG2E sweep");
}

}  // namespace kge
