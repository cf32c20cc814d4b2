// kge_proje.hip -- ProjE_pointwise (models/projection.py:128-257) trained on its labelled columns alone.
// For a row with entity e and relation r on side s (0: f1 = De1 / Dr1 / bc1 on (h, r), the "tail" direction; 1: f2 on (t, r)):
//     x   = tanh(ent[e] o De_s + rel[r] o Dr_s + bc_s) * m                       k_proje_body
//     z_c = <x, ent[c]>,  s = sigmoid(z_c),  u = 1 - s                            for the LABELLED columns c of the row only
//     loss = - sum_{y = +1} log(max(s, 1e-10)) - sum_{y = -1} log(max(u, 1e-10))
// The labels of a row are its positives (a CSR of ascending distinct ids) and ONE list of distinct negative ids shared by the whole
// batch; a negative that is a positive of the row is skipped (binary search).  The [B, E] product of the reference is never formed:
// the step works on B * n_neg + n_pos logits (n_neg <= 100 in the reference's generator).
//
//     k_proje_logits   one wave per labelled (row, column): the dot product, the loss term (double, into a term list) and dz
//     k_proje_dx       one wave per (row, 64 columns of x): dx = sum_c dz_c ent[c], the row's labels walked in list order
//     k_proje_gneg     one wave per (negative, 64 columns): g_ent[neg] += sum_b dz_b x_b, the batch walked in row order (no atomics:
//                      the ids of the list are distinct)
//     k_proje_gpos     one wave per positive entry: g_ent[c] += dz x_b with float atomics (256 contiguous bytes per instruction)
//     k_proje_body_bwd one wave per row: dpre = dx m (1 - tanh^2) -> workspace, g_ent[e] += dpre De_s, g_rel[r] += dpre Dr_s (atomics)
//     k_proje_rows     g_De_s, g_Dr_s, g_bc_s += sums of dpre ent[e], dpre rel[r], dpre over the batch in a FIXED order
//     k_proje_reg      lmbda sum |w| (double partials per workgroup) and g += lmbda sign(w) over ent, rel, De1, Dr1, De2, Dr2
//     k_proje_finish   one workgroup: the term list and the partials summed in double in a fixed order, ONE float added to the loss
// The product with the negative block is 2 B n_neg dim flops (8 MFLOP at the preset's shape): the step is bound by its launches and
// by the regulariser's sweep over the tables, so the products stay on the vector ALUs in the simplest shape that is coalesced.
//
// The dropout draw is the shared one (kge_projection.h spells the Philox counters out), with
//     elem    = the column j of x;   site = the side s;   row = position in the call's row list
#include "kge_projection.h"

namespace kge {

constexpr int kPjMaxDim = 2048;
constexpr float kPjClamp = 1e-10f;
constexpr int kPjRegBlocks = 512;     // workgroups (and double partials) of the regulariser's sweep
constexpr int kPjPhases = 16;         // row phases of k_proje_rows: 64 columns x 16 phases per workgroup

struct PjRng {
    DropKey key;
    uint32_t thr;
    float scale;
    int drop;
};
struct PjBody {
    const float *ent, *rel, *bc, *De, *Dr;
    float *g_ent, *g_rel, *g_bc, *g_De, *g_Dr;
    int dim, side;
    int64_t n;
    PjRng g;
};

// one wave per row: x[row] = tanh(ent[e] De + rel[r] Dr + bc) * m
__global__ void __launch_bounds__(256) k_proje_body(PjBody a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                    float* __restrict__ x) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n) return;
    const float* __restrict__ er = a.ent + e[row] * a.dim;
    const float* __restrict__ rr = a.rel + r[row] * a.dim;
    for (int j = lane; j < a.dim; j += 64) {
        float v = tanhf(er[j] * a.De[j] + rr[j] * a.Dr[j] + a.bc[j]);
        if (a.g.drop) v *= drop_row_factor(a.g.key, a.side, j, row, a.g.thr, a.g.scale);
        x[row * a.dim + j] = v;
    }
}

// one wave per row: dpre = dx * m * (1 - tanh^2) -> dpre[row]; the row's shares of g_ent[e] and g_rel[r] with float atomics
__global__ void __launch_bounds__(256) k_proje_body_bwd(PjBody a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                        const float* __restrict__ dx, float* __restrict__ dpre) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n) return;
    const int64_t eo = e[row] * a.dim, ro = r[row] * a.dim;
    for (int j = lane; j < a.dim; j += 64) {
        const float De = a.De[j], Dr = a.Dr[j];
        const float y = tanhf(a.ent[eo + j] * De + a.rel[ro + j] * Dr + a.bc[j]);
        float g = dx[row * a.dim + j];
        if (a.g.drop) g *= drop_row_factor(a.g.key, a.side, j, row, a.g.thr, a.g.scale);
        g *= 1.0f - y * y;
        dpre[row * a.dim + j] = g;
        unsafeAtomicAdd(a.g_ent + eo + j, g * De);
        unsafeAtomicAdd(a.g_rel + ro + j, g * Dr);
    }
}

// g_De[j] += sum_b dpre[b][j] ent[e_b][j], g_Dr[j] += sum_b dpre[b][j] rel[r_b][j], g_bc[j] += sum_b dpre[b][j].  A workgroup owns 64
// columns; thread (phase, column) adds the rows b = phase, phase + 16, ... in order and the 16 phase sums are added in phase order:
// the same association whatever the timing -- bit-identical run to run.
__global__ void __launch_bounds__(64 * kPjPhases) k_proje_rows(PjBody a, const int64_t* __restrict__ e, const int64_t* __restrict__ r,
                                                              const float* __restrict__ dpre) {
    __shared__ float part[3][kPjPhases][64];
    const int c = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int j = (int)blockIdx.x * 64 + c;
    float sd = 0.0f, sr = 0.0f, sb = 0.0f;
    if (j < a.dim)
        for (int64_t b = ph; b < a.n; b += kPjPhases) {
            const float g = dpre[b * a.dim + j];
            sd += g * a.ent[e[b] * a.dim + j];
            sr += g * a.rel[r[b] * a.dim + j];
            sb += g;
        }
    part[0][ph][c] = sd; part[1][ph][c] = sr; part[2][ph][c] = sb;
    __syncthreads();
    if (ph < 3 && j < a.dim) {
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < kPjPhases; ++q) s += part[ph][q][c];
        float* __restrict__ dst = ph == 0 ? a.g_De : ph == 1 ? a.g_Dr : a.g_bc;
        dst[j] += s;
    }
}

// the labelled entries of one direction: q < batch * n_neg is (row q / n_neg, negative q % n_neg), the rest are the positives in CSR order
struct PjLabels {
    const float *x, *ent;
    const int64_t* pos_off;
    const int32_t *pos_ids, *neg;
    int64_t batch, n_pos, n_neg, E;
    int dim;
};
__device__ __forceinline__ int64_t pj_row_of(const int64_t* __restrict__ off, int64_t batch, int64_t p) {   // the row b with off[b] <= p < off[b + 1]
    int64_t lo = 0, hi = batch - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256) k_proje_logits(PjLabels a, float* __restrict__ dz, double* __restrict__ terms) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nq = a.batch * a.n_neg + a.n_pos;
    if (q >= nq) return;   // (wave-uniform)
    const bool negative = q < a.batch * a.n_neg;
    int64_t b;
    int32_t c;
    bool live = true;
    if (negative) {
        b = q / a.n_neg;
        c = a.neg[q - b * a.n_neg];
        int64_t lo = a.pos_off[b], hi = a.pos_off[b + 1];
        while (lo < hi) {   // a negative that is a positive of the row carries the label +1: skipped here
            const int64_t mid = (lo + hi) >> 1;
            const int32_t v = a.pos_ids[mid];
            if (v == c) { live = false; break; }
            if (v < c) lo = mid + 1; else hi = mid;
        }
    } else {
        const int64_t p = q - a.batch * a.n_neg;
        b = pj_row_of(a.pos_off, a.batch, p);
        c = a.pos_ids[p];
    }
    if (c < 0 || (int64_t)c >= a.E) live = false;
    float g = 0.0f;
    double term = 0.0;
    if (live) {
        const float* __restrict__ xr = a.x + b * a.dim;
        const float* __restrict__ er = a.ent + (int64_t)c * a.dim;
        float z = 0.0f;
        for (int j = lane; j < a.dim; j += 64) z += xr[j] * er[j];
        z = wave_sum_xor(z);
        const float s = 1.0f / (1.0f + expf(-z));
        const float u = 1.0f - s;
        if (negative) {
            term = (double)-logf(fmaxf(u, kPjClamp));
            g = u > kPjClamp ? s : 0.0f;
        } else {
            term = (double)-logf(fmaxf(s, kPjClamp));
            g = s > kPjClamp ? -u : 0.0f;
        }
    }
    if (lane == 0) { dz[q] = g; terms[q] = term; }
}

// dx[b][j] = sum over the row's labelled columns of dz ent[c][j]: the negatives in list order, then the positives in CSR order
__global__ void __launch_bounds__(256) k_proje_dx(PjLabels a, const float* __restrict__ dz, float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int chunks = (a.dim + 63) / 64;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= a.batch * chunks) return;
    const int64_t b = item / chunks;
    const int j = (int)(item - b * chunks) * 64 + lane;
    const int jc = min(j, a.dim - 1);
    float acc = 0.0f;
    const float* __restrict__ dn = dz + b * a.n_neg;
    for (int64_t i = 0; i < a.n_neg; ++i) {
        const float g = dn[i];
        if (g != 0.0f) acc += g * a.ent[(int64_t)a.neg[i] * a.dim + jc];   // (g == 0: skipped, clamped or an id out of range)
    }
    const float* __restrict__ dp = dz + a.batch * a.n_neg;
    for (int64_t p = a.pos_off[b]; p < a.pos_off[b + 1]; ++p) {
        const float g = dp[p];
        if (g != 0.0f) acc += g * a.ent[(int64_t)a.pos_ids[p] * a.dim + jc];
    }
    if (j < a.dim) dx[b * a.dim + j] = acc;
}

// g_ent[neg_i][j] += sum_b dz[b][i] x[b][j], b in row order; the ids of the list are distinct, so every destination has one owner
__global__ void __launch_bounds__(256) k_proje_gneg(PjLabels a, const float* __restrict__ dz, float* __restrict__ g_ent) {
    const int lane = threadIdx.x & 63;
    const int chunks = (a.dim + 63) / 64;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= a.n_neg * chunks) return;
    const int64_t i = item / chunks;
    const int j = (int)(item - i * chunks) * 64 + lane;
    const int jc = min(j, a.dim - 1);
    const int32_t c = a.neg[i];
    if (c < 0 || (int64_t)c >= a.E) return;
    float acc = 0.0f;
    for (int64_t b = 0; b < a.batch; ++b) {
        const float g = dz[b * a.n_neg + i];
        if (g != 0.0f) acc += g * a.x[b * a.dim + jc];
    }
    if (j < a.dim) g_ent[(int64_t)c * a.dim + j] += acc;
}

// one wave per positive entry: g_ent[c] += dz x_b
__global__ void __launch_bounds__(256) k_proje_gpos(PjLabels a, const float* __restrict__ dz, float* __restrict__ g_ent) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.n_pos) return;
    const float g = dz[a.batch * a.n_neg + p];
    if (g == 0.0f) return;   // (clamped or an id out of range)
    const int64_t b = pj_row_of(a.pos_off, a.batch, p);
    float* __restrict__ dst = g_ent + (int64_t)a.pos_ids[p] * a.dim;
    const float* __restrict__ xr = a.x + b * a.dim;
    for (int j = lane; j < a.dim; j += 64) unsafeAtomicAdd(dst + j, g * xr[j]);
}

struct PjRegSeg {
    const float* w;
    float* g;
    int64_t end;   // running end of the segment in the sweep's flat index
};
struct PjReg {
    PjRegSeg seg[6];
    int64_t total;
    float lmbda;
};
__device__ __forceinline__ double pj_block_sum(double v, double* sh) {   // fixed tree over the workgroup; the result is valid in thread 0
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = (int)blockDim.x >> 1; o >= 1; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    return sh[0];
}
__global__ void __launch_bounds__(256) k_proje_reg(PjReg a, double* __restrict__ partials) {
    __shared__ double sh[256];
    double sum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
        const float* __restrict__ wp = a.seg[0].w;   // (selects with constant indices: a lane-dependent index would put the list in scratch)
        float* __restrict__ gp = a.seg[0].g;
        int64_t base = 0;
#pragma unroll
        for (int q = 1; q < 6; ++q)
            if (i >= a.seg[q - 1].end) { wp = a.seg[q].w; gp = a.seg[q].g; base = a.seg[q - 1].end; }
        const float w = wp[i - base];
        sum += (double)fabsf(w);
        if (w != 0.0f) gp[i - base] += w > 0.0f ? a.lmbda : -a.lmbda;
    }
    const double tot = pj_block_sum(sum, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = (double)a.lmbda * tot;
}

// loss += the sum of `n` doubles, in a fixed order, as ONE float
__global__ void __launch_bounds__(1024) k_proje_finish(const double* __restrict__ terms, int64_t n, float* __restrict__ loss) {
    __shared__ double sh[1024];
    double sum = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) sum += terms[i];
    const double tot = pj_block_sum(sum, sh);
    if (threadIdx.x == 0) unsafeAtomicAdd(loss, (float)tot);
}

// ------------------------------------------------------------------------------------------------------------------ host side
static int pj_check(const kge_proje_desc* d, const char* who, bool grads) {
    if (!d) { set_error("%s: null descriptor", who); return -1; }
    if (!d->ent || !d->rel || !d->bc1 || !d->De1 || !d->Dr1 || !d->bc2 || !d->De2 || !d->Dr2) {
        set_error("%s: null tables (ent, rel, bc1, De1, Dr1, bc2, De2 and Dr2 are all required)", who);
        return -1;
    }
    if (d->tot_entity <= 0 || d->tot_relation <= 0 || d->dim <= 0) {
        set_error("%s: tot_entity, tot_relation and dim must be positive (got %lld, %lld, %d)", who, (long long)d->tot_entity,
                  (long long)d->tot_relation, d->dim);
        return -1;
    }
    if (d->dim > kPjMaxDim) { set_error("%s: dim = %d exceeds %d", who, d->dim, kPjMaxDim); return -1; }
    if (d->tot_entity > 2147483647LL) { set_error("%s: tot_entity = %lld: label ids are int32", who, (long long)d->tot_entity); return -1; }
    if (drop_check(who, &d->hidden_dropout, 1, d->offset)) return -1;
    if (grads && (!d->g_ent || !d->g_rel || !d->g_bc1 || !d->g_De1 || !d->g_Dr1 || !d->g_bc2 || !d->g_De2 || !d->g_Dr2)) {
        set_error("%s: null gradient buffers (all eight are required)", who);
        return -1;
    }
    return 0;
}
static int pj_side_check(const char* who, int side) {
    if (side != 0 && side != 1) { set_error("%s: side must be 0 (tail direction) or 1 (head direction), got %d", who, side); return -1; }
    return 0;
}

static PjBody pj_body(const kge_proje_desc* d, int side, int64_t n) {
    PjBody a{};
    a.ent = d->ent; a.rel = d->rel;
    a.bc = side ? d->bc2 : d->bc1; a.De = side ? d->De2 : d->De1; a.Dr = side ? d->Dr2 : d->Dr1;
    a.g_ent = d->g_ent; a.g_rel = d->g_rel;
    a.g_bc = side ? d->g_bc2 : d->g_bc1; a.g_De = side ? d->g_De2 : d->g_De1; a.g_Dr = side ? d->g_Dr2 : d->g_Dr1;
    a.dim = d->dim; a.side = side; a.n = n;
    a.g.key = drop_key(d->seed, d->offset);
    a.g.thr = drop_thr(d->hidden_dropout);
    a.g.scale = drop_scale(d->hidden_dropout);
    a.g.drop = d->train != 0 && d->hidden_dropout > 0.0f;
    return a;
}

static int pj_forward(const kge_proje_desc* d, const int64_t* e, const int64_t* r, int64_t n, int side, float* x, hipStream_t s) {
    hipLaunchKernelGGL(k_proje_body, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, pj_body(d, side, n), e, r, x);
    return check_launch("k_proje_body");
}
static size_t pj_bwd_bytes(const kge_proje_desc* d, int64_t n) { return align256((size_t)n * d->dim * sizeof(float)); }
static int pj_backward(const kge_proje_desc* d, const int64_t* e, const int64_t* r, int64_t n, int side, const float* dx, void* ws,
                       hipStream_t s) {
    const PjBody a = pj_body(d, side, n);
    float* dpre = (float*)ws;
    hipLaunchKernelGGL(k_proje_body_bwd, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, a, e, r, dx, dpre);
    hipLaunchKernelGGL(k_proje_rows, dim3((unsigned)((d->dim + 63) / 64)), dim3(64 * kPjPhases), 0, s, a, e, r, dpre);
    return check_launch("k_proje_body_bwd / k_proje_rows");
}

// one direction's labelled entries: dz float [B * n_neg + n_pos] and as many double terms
static int64_t pj_entries(int64_t B, int64_t n_pos, int64_t n_neg) { return B * n_neg + n_pos; }
static size_t pj_dz_bytes(int64_t B, int64_t n_pos, int64_t n_neg) { return align256((size_t)(pj_entries(B, n_pos, n_neg) + 1) * sizeof(float)); }
static size_t pj_term_bytes(int64_t B, int64_t n_pos, int64_t n_neg) { return align256((size_t)(pj_entries(B, n_pos, n_neg) + 1) * sizeof(double)); }

// logits, dx and the two g_ent passes of one direction; the terms of the entries are left in `terms` for k_proje_finish
static int pj_labels(const float* x, int64_t B, int dim, const float* ent, int64_t E, const int64_t* off, const int32_t* ids, int64_t n_pos,
                     const int32_t* neg, int64_t n_neg, float* dz, double* terms, float* dx, float* g_ent, hipStream_t s) {
    PjLabels a{};
    a.x = x; a.ent = ent; a.pos_off = off; a.pos_ids = ids; a.neg = neg;
    a.batch = B; a.n_pos = n_pos; a.n_neg = n_neg; a.E = E; a.dim = dim;
    const int64_t nq = pj_entries(B, n_pos, n_neg);
    const int chunks = (dim + 63) / 64;
    if (nq > 0) hipLaunchKernelGGL(k_proje_logits, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, a, dz, terms);
    hipLaunchKernelGGL(k_proje_dx, dim3((unsigned)((B * chunks + 3) / 4)), dim3(256), 0, s, a, dz, dx);
    if (int rc = check_launch("k_proje_logits / k_proje_dx")) return rc;
    if (n_neg > 0) hipLaunchKernelGGL(k_proje_gneg, dim3((unsigned)((n_neg * chunks + 3) / 4)), dim3(256), 0, s, a, dz, g_ent);
    if (n_pos > 0) hipLaunchKernelGGL(k_proje_gpos, dim3((unsigned)((n_pos + 3) / 4)), dim3(256), 0, s, a, dz, g_ent);
    return check_launch("k_proje_gneg / k_proje_gpos");
}
static int pj_label_args_ok(int64_t B, int64_t n_pos, int64_t n_neg) {
    // grids are counted in 32 bits: (entries + 3) / 4 workgroups
    return B >= 0 && n_pos >= 0 && n_neg >= 0 && n_neg <= (1 << 20) && B <= (1 << 24) && n_pos <= (1LL << 31) &&
           pj_entries(B, n_pos, n_neg) <= (1LL << 32);
}

// fused step: x [2, B, dim] | dx [2, B, dim] | dpre [B, dim] | dz (the larger direction) | terms: direction 0, direction 1, regulariser
struct PjStepPlan {
    size_t x, dx, dpre, dz, terms, total;
    int64_t t1, treg, nterms;   // starts of direction 1's terms and of the regulariser's partials, and their count
};
static PjStepPlan pj_step_plan(const kge_proje_desc* d, int64_t B, int64_t n_hr, int64_t n_tr, int64_t n_neg) {
    PjStepPlan p{};
    const size_t xb = align256((size_t)2 * B * d->dim * sizeof(float));
    p.x = 0;
    p.dx = xb;
    p.dpre = p.dx + xb;
    p.dz = p.dpre + pj_bwd_bytes(d, B);
    p.terms = p.dz + pj_dz_bytes(B, n_hr > n_tr ? n_hr : n_tr, n_neg);
    p.t1 = pj_entries(B, n_hr, n_neg);
    p.treg = p.t1 + pj_entries(B, n_tr, n_neg);
    p.nterms = p.treg + kPjRegBlocks;
    p.total = p.terms + align256((size_t)p.nterms * sizeof(double));
    return p;
}

// the rank pass's body (kge_projection.hip): predict_tail_rank / predict_head_rank, so no dropout; f1 on the h rows, f2 on the t rows
static int pj_eval_body(const void* desc, const int64_t* e, const int64_t* r, int64_t n, float* x, void*, size_t, hipStream_t s) {
    kge_proje_desc ev = *(const kge_proje_desc*)desc;
    ev.train = 0;
    if (int rc = pj_forward(&ev, e, r, n, 0, x, s)) return rc;
    return pj_forward(&ev, e + n, r + n, n, 1, x + n * ev.dim, s);
}
static ProjectionEval pj_eval(const kge_proje_desc* d) {
    return ProjectionEval{d->dim, d->tot_entity, d->tot_relation, d->ent, 0, pj_eval_body};
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_proje_body_forward_workspace_bytes(const kge_proje_desc* d, int64_t n) {
    return pj_check(d, "kge_proje_body_forward_workspace_bytes", false) || n < 0 ? 0 : 256;   // (none needed: a token size, so that 0 = refused)
}

int kge_proje_body_forward(const kge_proje_desc* d, const int64_t* e, const int64_t* r, int64_t n, int32_t side, float* x, void* workspace,
                           size_t workspace_bytes, void* stream) {
    const char* who = "kge_proje_body_forward";
    if (pj_check(d, who, false) || pj_side_check(who, side)) return -1;
    if (n < 0 || n > (1LL << 33) || (n > 0 && (!e || !r || !x))) { set_error("%s: bad arguments", who); return -1; }
    if (ws_check(who, workspace, workspace_bytes, 256)) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_er_ids(who, d->tot_entity, d->tot_relation, e, r, n, s)) return rc;
    return pj_forward(d, e, r, n, side, x, s);
}

size_t kge_proje_body_backward_workspace_bytes(const kge_proje_desc* d, int64_t n) {
    return pj_check(d, "kge_proje_body_backward_workspace_bytes", false) || n < 0 ? 0 : pj_bwd_bytes(d, n > 0 ? n : 1);
}

int kge_proje_body_backward(const kge_proje_desc* d, const int64_t* e, const int64_t* r, int64_t n, int32_t side, const float* dx,
                            void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_proje_body_backward";
    if (pj_check(d, who, true) || pj_side_check(who, side)) return -1;
    if (n < 0 || n > (1LL << 33) || (n > 0 && (!e || !r || !dx))) { set_error("%s: bad arguments", who); return -1; }
    if (ws_check(who, workspace, workspace_bytes, pj_bwd_bytes(d, n > 0 ? n : 1))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_er_ids(who, d->tot_entity, d->tot_relation, e, r, n, s)) return rc;
    return pj_backward(d, e, r, n, side, dx, workspace, s);
}

size_t kge_proje_label_loss_workspace_bytes(int64_t batch, int32_t dim, int64_t n_pos, int64_t n_neg) {
    if (dim <= 0 || dim > kPjMaxDim || !pj_label_args_ok(batch, n_pos, n_neg)) {
        set_error("kge_proje_label_loss_workspace_bytes: bad sizes (batch %lld, dim %d, n_pos %lld, n_neg %lld)", (long long)batch, dim,
                  (long long)n_pos, (long long)n_neg);
        return 0;
    }
    return pj_dz_bytes(batch, n_pos, n_neg) + pj_term_bytes(batch, n_pos, n_neg);
}

int kge_proje_label_loss(const float* x, int64_t batch, int32_t dim, const float* ent, int64_t tot_entity, const int64_t* pos_off,
                         const int32_t* pos_ids, int64_t n_pos, const int32_t* neg, int64_t n_neg, void* workspace, size_t workspace_bytes,
                         float* loss, float* dx, float* g_ent, void* stream) {
    const char* who = "kge_proje_label_loss";
    if (dim <= 0 || dim > kPjMaxDim) { set_error("%s: dim = %d must be in 1..%d", who, dim, kPjMaxDim); return -1; }
    if (!pj_label_args_ok(batch, n_pos, n_neg) || tot_entity <= 0 || tot_entity > 2147483647LL || !ent || !loss ||
        (batch > 0 && (!x || !pos_off || !dx || !g_ent)) || (n_pos > 0 && !pos_ids) || (n_neg > 0 && !neg)) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    if (ws_check(who, workspace, workspace_bytes, pj_dz_bytes(batch, n_pos, n_neg) + pj_term_bytes(batch, n_pos, n_neg))) return -1;
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (n_pos > 0)
        if (int rc = debug_check_ids32(who, "positive", pos_ids, n_pos, 1, 0, tot_entity, s)) return rc;
    if (n_neg > 0)
        if (int rc = debug_check_ids32(who, "negative", neg, n_neg, 1, 0, tot_entity, s)) return rc;
    float* dz = (float*)workspace;
    double* terms = (double*)((char*)workspace + pj_dz_bytes(batch, n_pos, n_neg));
    if (int rc = pj_labels(x, batch, dim, ent, tot_entity, pos_off, pos_ids, n_pos, neg, n_neg, dz, terms, dx, g_ent, s)) return rc;
    const int64_t nq = pj_entries(batch, n_pos, n_neg);
    if (nq > 0) hipLaunchKernelGGL(k_proje_finish, dim3(1), dim3(1024), 0, s, terms, nq, loss);
    return check_launch("k_proje_finish");
}

size_t kge_proje_train_workspace_bytes(const kge_proje_desc* d, int64_t batch, int64_t n_hr, int64_t n_tr, int64_t n_neg) {
    const char* who = "kge_proje_train_workspace_bytes";
    if (pj_check(d, who, false)) return 0;
    if (!pj_label_args_ok(batch, n_hr, n_neg) || !pj_label_args_ok(batch, n_tr, n_neg)) { set_error("%s: bad sizes", who); return 0; }
    return pj_step_plan(d, batch > 0 ? batch : 1, n_hr, n_tr, n_neg).total;
}

int kge_proje_train(const kge_proje_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t batch, const int64_t* hr_off,
                    const int32_t* hr_ids, int64_t n_hr, const int64_t* tr_off, const int32_t* tr_ids, int64_t n_tr, const int32_t* neg,
                    int64_t n_neg, float lmbda, void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    const char* who = "kge_proje_train";
    if (pj_check(d, who, true)) return -1;
    if (!pj_label_args_ok(batch, n_hr, n_neg) || !pj_label_args_ok(batch, n_tr, n_neg) || !loss ||
        (batch > 0 && (!h || !r || !t || !hr_off || !tr_off)) || (n_hr > 0 && !hr_ids) || (n_tr > 0 && !tr_ids) || (n_neg > 0 && !neg)) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    const PjStepPlan p = pj_step_plan(d, batch > 0 ? batch : 1, n_hr, n_tr, n_neg);
    if (ws_check(who, workspace, workspace_bytes, p.total)) return -1;
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t B = batch;
    const int dim = d->dim;
    const int64_t E = d->tot_entity;
    if (int rc = check_er_ids(who, d->tot_entity, d->tot_relation, h, r, B, s)) return rc;
    if (int rc = debug_check_ids(who, "entity", t, B, 1, 0, E, s)) return rc;
    if (n_hr > 0)
        if (int rc = debug_check_ids32(who, "hr_t label", hr_ids, n_hr, 1, 0, E, s)) return rc;
    if (n_tr > 0)
        if (int rc = debug_check_ids32(who, "tr_h label", tr_ids, n_tr, 1, 0, E, s)) return rc;
    if (n_neg > 0)
        if (int rc = debug_check_ids32(who, "negative", neg, n_neg, 1, 0, E, s)) return rc;
    char* ws = (char*)workspace;
    float *x = (float*)(ws + p.x), *dx = (float*)(ws + p.dx), *dz = (float*)(ws + p.dz);
    double* terms = (double*)(ws + p.terms);
    // forward(h, r, hr_t, "tail") + forward(t, r, tr_h, "head") (utils/trainer.py:159-174): each direction numbers its own rows from 0
    if (int rc = pj_forward(d, h, r, B, 0, x, s)) return rc;
    if (int rc = pj_forward(d, t, r, B, 1, x + B * dim, s)) return rc;
    if (int rc = pj_labels(x, B, dim, d->ent, E, hr_off, hr_ids, n_hr, neg, n_neg, dz, terms, dx, d->g_ent, s)) return rc;
    if (int rc = pj_labels(x + B * dim, B, dim, d->ent, E, tr_off, tr_ids, n_tr, neg, n_neg, dz, terms + p.t1, dx + B * dim, d->g_ent, s)) return rc;
    if (int rc = pj_backward(d, h, r, B, 0, dx, ws + p.dpre, s)) return rc;
    if (int rc = pj_backward(d, t, r, B, 1, dx + B * dim, ws + p.dpre, s)) return rc;
    // + get_reg: lmbda (sum |De1| + |Dr1| + |De2| + |Dr2| + |ent| + |rel|), after every kernel that adds to these gradients with atomics
    PjReg g{};
    const float* w[6] = {d->ent, d->rel, d->De1, d->Dr1, d->De2, d->Dr2};
    float* gw[6] = {d->g_ent, d->g_rel, d->g_De1, d->g_Dr1, d->g_De2, d->g_Dr2};
    const int64_t numel[6] = {E * dim, d->tot_relation * dim, dim, dim, dim, dim};
    int64_t end = 0;
    for (int q = 0; q < 6; ++q) {
        end += numel[q];
        g.seg[q] = PjRegSeg{w[q], gw[q], end};
    }
    g.total = end;
    g.lmbda = lmbda;
    hipLaunchKernelGGL(k_proje_reg, dim3(kPjRegBlocks), dim3(256), 0, s, g, terms + p.treg);
    hipLaunchKernelGGL(k_proje_finish, dim3(1), dim3(1024), 0, s, terms, p.nterms, loss);
    return check_launch("k_proje_reg / k_proje_finish");
}

size_t kge_proje_eval_ranks_workspace_bytes(const kge_proje_desc* d, int64_t n) {
    return pj_check(d, "kge_proje_eval_ranks_workspace_bytes", false) || n < 0 ? 0 : projection_eval_workspace_bytes(pj_eval(d), n);
}

int kge_proje_eval_ranks(const kge_proje_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                         const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks,
                         int32_t* ties, void* stream) {
    const char* who = "kge_proje_eval_ranks";
    if (pj_check(d, who, false)) return -1;
    return projection_eval_ranks(who, pj_eval(d), d, triples, n, tail_off, tail_ids, head_off, head_ids, workspace, workspace_bytes, ranks,
                                 ties, stream);
}

}  // extern "C"
