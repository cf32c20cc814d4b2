// kge_tsne.hip -- t-SNE projection of embedding rows to 2-D: the perplexity search over the neighbour lists of kge_knn_rows, one
// evaluation of the gradient over the sparse joint probabilities, and the descent loop.  The repulsive term is an all-pairs sweep
// over the 2-D points; nothing in it is approximated (no Barnes-Hut tree, no interpolation grid).
//
//   k_tsne_affinities  one wave per row, at most two neighbours per lane: the binary search of the row's precision beta in float64
//                      (the reference implementation's: doubled or halved while a bound is open, bisected after, 100 steps at most,
//                      stop at |H - log perplexity| <= 1e-5), the row's smallest squared distance subtracted first.  Sums are xor
//                      butterflies: a fixed order.
//   k_tsne_repulse     workgroup (b, s) owns points i = 256 b + lane and slab s of the j range: tiles of 256 points go through two LDS
//                      buffers (one barrier per tile; every lane reads the same address, a broadcast), the lane keeps its point and
//                      four independent accumulator sets in registers.  Per pair: two subtractions, two FMAs for 1 + d^2, one
//                      v_rcp_f32, the accumulations.  The diagonal tile (uniform branch) zeroes w at j == i; points past n are
//                      (1e30, 0): d^2 overflows to +inf, w is exactly 0 and 0 * 1e30 is 0.  Writes (fx, fy, sum w) per (s, i) and the
//                      workgroup's float64 sum of w; no atomics.
//   k_tsne_attract     32 lanes per row walk the row's CSR entries (8-byte gathers of y_j), every workgroup re-sums the float64
//                      workgroup sums of the sweep in the same order into Z, the slabs' forces are added in slab order, and the
//                      gradient is finished.  UPDATE: the descent step (gains, update, Y) rides along and writes the other Y buffer.
//                      RECORD: the row's KL terms and |grad|^2 in float64, one pair per workgroup.
//   k_tsne_record      one workgroup: the pairs of k_tsne_attract in a fixed order -> (KL, |grad|_2).
// Launches per iteration: k_tsne_repulse, k_tsne_attract, and k_tsne_record where a record is asked for.
#include <cstdio>
#include <cmath>
#include "kge_internal.h"

namespace kge {

namespace {

constexpr int kTsneBlock = 256;
constexpr int kTsneWaves = kTsneBlock / 64;
constexpr int kTsneTile = KGE_TSNE_TILE;       // points per i block and per j tile: the diagonal tile of block b is tile b
constexpr int kTsneMaxSplit = 64;
constexpr int kTsneTargetGroups = 1024;        // the split fills the device: four workgroups of 256 per CU
constexpr int kTsneRowLanes = 32;              // lanes per CSR row in k_tsne_attract
constexpr int kTsneRowsPer = kTsneBlock / kTsneRowLanes;
constexpr int kTsneAttractMax = 1024;          // most workgroups of k_tsne_attract: each re-sums Z and leaves one record pair
constexpr float kTsnePad = 1e30f;              // x of the points past n: (y_i - 1e30)^2 = +inf, 1 / inf = 0, 0 * 1e30 = 0

static_assert(kTsneTile == kTsneBlock, "a lane owns one point of the i block and fills one place of the j tile");

__device__ __forceinline__ double tsne_wave_sum(double s) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

__device__ __forceinline__ double tsne_wave_min(double s) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const double o = __shfl_xor(s, d); s = o < s ? o : s; }
    return s;
}

// the workgroup's sum of one double per lane in a fixed order: butterfly per wave, the waves' sums left to right; valid in thread 0
__device__ __forceinline__ double tsne_block_sum(double v, double* s_w) {
    v = tsne_wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
    __syncthreads();
    return r;
}

}  // namespace

__global__ void __launch_bounds__(kTsneBlock) k_tsne_affinities(const float* __restrict__ dist, const int32_t* __restrict__ count, int64_t n,
                                                                  int k, double log_perp, float* __restrict__ cond_p,
                                                                  float* __restrict__ beta_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kTsneWaves + (threadIdx.x >> 6);
    if (row >= n) return;                                   // (a whole wave leaves: the butterflies below see full waves)
    int cnt = count[row];
    cnt = cnt < 0 ? 0 : (cnt > k ? k : cnt);
    const float* __restrict__ drow = dist + row * k;
    const bool live0 = lane < cnt, live1 = lane + 64 < cnt;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double d0 = inf, d1 = inf;
    if (live0) { const double d = (double)drow[lane]; d0 = d * d; }
    if (live1) { const double d = (double)drow[lane + 64]; d1 = d * d; }
    const double dmin = tsne_wave_min(d0 < d1 ? d0 : d1);
    d0 = live0 ? d0 - dmin : 0.0;
    d1 = live1 ? d1 - dmin : 0.0;
    double beta = 1.0, lo = -inf, hi = inf, p0 = 0.0, p1 = 0.0;
    if (cnt > 0) {
        for (int step = 0; step < 100; ++step) {            // (every lane holds the same sums: the trip count is the wave's)
            p0 = live0 ? exp(-d0 * beta) : 0.0;
            p1 = live1 ? exp(-d1 * beta) : 0.0;
            const double sum = tsne_wave_sum(p0 + p1);      // >= 1: the nearest neighbour's term
            p0 /= sum;
            p1 /= sum;
            const double dp = tsne_wave_sum(d0 * p0 + d1 * p1);
            const double diff = log(sum) + beta * dp - log_perp;
            if (fabs(diff) <= 1e-5) break;
            if (diff > 0.0) { lo = beta; beta = hi == inf ? beta * 2.0 : (beta + hi) * 0.5; }
            else { hi = beta; beta = lo == -inf ? beta * 0.5 : (beta + lo) * 0.5; }
        }
    }
    if (lane < k) cond_p[row * k + lane] = (float)p0;
    if (lane + 64 < k) cond_p[row * k + lane + 64] = (float)p1;
    if (lane == 0) beta_out[row] = (float)beta;
}

// four points of one tile against the lane's point: accumulator set u takes the points 4 m + u
template <bool DIAG>
__device__ __forceinline__ void tsne_tile(const float4* __restrict__ sX, const float4* __restrict__ sY, float xi, float yi, int self,
                                          float (&fx)[4], float (&fy)[4], float (&sw)[4]) {
#pragma unroll 2
    for (int m = 0; m < kTsneTile / 4; ++m) {
        const float4 a = sX[m], b = sY[m];
        const float px[4] = {a.x, a.y, a.z, a.w}, py[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float dx = xi - px[u], dy = yi - py[u];
            float w = __builtin_amdgcn_rcpf(fmaf(dy, dy, fmaf(dx, dx, 1.0f)));
            if (DIAG) w = (4 * m + u == self) ? 0.0f : w;
            const float w2 = w * w;
            sw[u] += w;
            fx[u] = fmaf(w2, dx, fx[u]);
            fy[u] = fmaf(w2, dy, fy[u]);
        }
    }
}

__global__ void __launch_bounds__(kTsneBlock) k_tsne_repulse(const float2* __restrict__ Y, int n, int tiles_per, int jtiles,
                                                               float4* __restrict__ part, double* __restrict__ zpart) {
    __shared__ float4 s_x[2][kTsneTile / 4], s_y[2][kTsneTile / 4];   // the tile's x and y apart: four points per 16-byte read
    __shared__ double s_w[kTsneWaves];
    const int tid = threadIdx.x;
    const int S = gridDim.y, sp = blockIdx.y;
    const int t0 = sp * tiles_per, t1 = (t0 + tiles_per < jtiles) ? t0 + tiles_per : jtiles;   // t0 < t1: no slab is empty
    const int i = blockIdx.x * kTsneTile + tid;
    const float2 yi = Y[i < n ? i : n - 1];
    float fx[4] = {0.f, 0.f, 0.f, 0.f}, fy[4] = {0.f, 0.f, 0.f, 0.f}, sw[4] = {0.f, 0.f, 0.f, 0.f};

    auto load = [&](int t) __attribute__((always_inline)) {
        const int j = t * kTsneTile + tid;
        float2 v = Y[j < n ? j : n - 1];                   // an unconditional load from a clamped address, then the select
        if (j >= n) { v.x = kTsnePad; v.y = 0.f; }
        return v;
    };
    float2 nxt = load(t0);
    reinterpret_cast<float*>(s_x[0])[tid] = nxt.x;
    reinterpret_cast<float*>(s_y[0])[tid] = nxt.y;
    __syncthreads();
    int cur = 0;
    for (int t = t0; t < t1; ++t) {
        if (t + 1 < t1) nxt = load(t + 1);
        if (t == (int)blockIdx.x) tsne_tile<true>(s_x[cur], s_y[cur], yi.x, yi.y, tid, fx, fy, sw);
        else tsne_tile<false>(s_x[cur], s_y[cur], yi.x, yi.y, -1, fx, fy, sw);
        if (t + 1 < t1) { reinterpret_cast<float*>(s_x[cur ^ 1])[tid] = nxt.x; reinterpret_cast<float*>(s_y[cur ^ 1])[tid] = nxt.y; }
        __syncthreads();                                    // tile t is consumed and tile t + 1 is in place
        cur ^= 1;
    }
    const float rx = (fx[0] + fx[1]) + (fx[2] + fx[3]), ry = (fy[0] + fy[1]) + (fy[2] + fy[3]);
    const float rw = (sw[0] + sw[1]) + (sw[2] + sw[3]);
    if (i < n) part[(size_t)sp * n + i] = make_float4(rx, ry, rw, 0.f);
    const double z = tsne_block_sum(i < n ? (double)rw : 0.0, s_w);
    if (tid == 0) zpart[(size_t)blockIdx.x * S + sp] = z;
}

template <bool UPDATE, bool RECORD>
__global__ void __launch_bounds__(kTsneBlock) k_tsne_attract(const float2* __restrict__ Y, int n, const int64_t* __restrict__ row_off,
                                                               const int32_t* __restrict__ col, const float* __restrict__ val,
                                                               float exaggeration, const float4* __restrict__ part, int S,
                                                               const double* __restrict__ zpart, int nz, float2* __restrict__ grad,
                                                               double* __restrict__ z_out, float2* __restrict__ y_new,
                                                               float2* __restrict__ update, float2* __restrict__ gains, float momentum,
                                                               float learning_rate, double* __restrict__ blockpart) {
    __shared__ double s_w[kTsneWaves];
    __shared__ double s_z;
    const int tid = threadIdx.x, sub = tid & (kTsneRowLanes - 1);
    // Z: every workgroup adds the sweep's workgroup sums in the same order
    double zl = 0.0;
    for (int t = tid; t < nz; t += kTsneBlock) zl += zpart[t];
    zl = tsne_block_sum(zl, s_w);
    if (tid == 0) { s_z = zl; if (blockIdx.x == 0 && z_out) *z_out = zl; }
    __syncthreads();
    const double Z = s_z;
    double kl = 0.0, g2 = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * kTsneRowsPer; base < n; base += (int64_t)gridDim.x * kTsneRowsPer) {
        const int i = (int)base + tid / kTsneRowLanes;      // (n <= 2^31 - 257: base + 7 fits)
        const bool ok = i < n;
        const float2 yi = Y[ok ? i : n - 1];
        const int64_t e0 = ok ? row_off[i] : 0, e1 = ok ? row_off[i + 1] : 0;
        float ax = 0.f, ay = 0.f;
        for (int64_t e = e0 + sub; e < e1; e += 2 * kTsneRowLanes) {
            // two entries per trip, so that their gathers are in flight together; a missing second entry is the first with P = 0
            const int64_t e2 = e + kTsneRowLanes < e1 ? e + kTsneRowLanes : e;
            const float p[2] = {val[e], e2 != e ? val[e2] : 0.f};
            const float2 yj[2] = {Y[col[e]], Y[col[e2]]};
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float dx = yi.x - yj[u].x, dy = yi.y - yj[u].y;
                const float q = fmaf(dy, dy, fmaf(dx, dx, 1.0f));
                const float pw = p[u] / q;
                ax = fmaf(pw, dx, ax);
                ay = fmaf(pw, dy, ay);
                if (RECORD) { if (p[u] > 0.f) kl += (double)p[u] * log((double)p[u] * (double)q * Z); }
            }
        }
#pragma unroll
        for (int d = kTsneRowLanes / 2; d > 0; d >>= 1) { ax += __shfl_xor(ax, d, kTsneRowLanes); ay += __shfl_xor(ay, d, kTsneRowLanes); }
        if (ok && sub == 0) {
            double rx = 0.0, ry = 0.0;
            for (int s = 0; s < S; ++s) { const float4 f = part[(size_t)s * n + i]; rx += (double)f.x; ry += (double)f.y; }
            const float qx = (float)(rx / Z), qy = (float)(ry / Z);
            const float gx = 4.0f * (exaggeration * ax - qx), gy = 4.0f * (exaggeration * ay - qy);
            if (grad) grad[i] = make_float2(gx, gy);
            if (RECORD) g2 += (double)gx * (double)gx + (double)gy * (double)gy;
            if (UPDATE) {
                float2 u = update[i], g = gains[i];
                g.x = (u.x * gx < 0.f) ? g.x + 0.2f : g.x * 0.8f;
                g.y = (u.y * gy < 0.f) ? g.y + 0.2f : g.y * 0.8f;
                g.x = g.x < 0.01f ? 0.01f : g.x;
                g.y = g.y < 0.01f ? 0.01f : g.y;
                u.x = momentum * u.x - learning_rate * (g.x * gx);
                u.y = momentum * u.y - learning_rate * (g.y * gy);
                gains[i] = g;
                update[i] = u;
                y_new[i] = make_float2(yi.x + u.x, yi.y + u.y);
            }
        }
    }
    if (RECORD) {
        const double a = tsne_block_sum(kl, s_w), b = tsne_block_sum(g2, s_w);
        if (tid == 0) { blockpart[2 * blockIdx.x] = a; blockpart[2 * blockIdx.x + 1] = b; }
    }
}

__global__ void __launch_bounds__(kTsneBlock) k_tsne_record(const double* __restrict__ blockpart, int nb, double* __restrict__ kl_out,
                                                              double* __restrict__ gnorm_out) {
    __shared__ double s_w[kTsneWaves];
    double a = 0.0, b = 0.0;
    for (int t = threadIdx.x; t < nb; t += kTsneBlock) { a += blockpart[2 * t]; b += blockpart[2 * t + 1]; }
    a = tsne_block_sum(a, s_w);
    b = tsne_block_sum(b, s_w);
    if (threadIdx.x == 0) { if (kl_out) *kl_out = a; if (gnorm_out) *gnorm_out = sqrt(b); }
}

namespace {

struct TsnePlan { int ib, tiles_per, S, ab; size_t part_bytes, zpart_bytes, bytes; };

// The slab split is a function of n alone: enough slabs that the i blocks fill the device, whole tiles, none empty; KGE_TSNE_SPLIT
// forces it (tests).
TsnePlan tsne_plan(int64_t n) {
    TsnePlan p;
    p.ib = (int)((n + kTsneTile - 1) / kTsneTile);
    int most = p.ib < kTsneMaxSplit ? p.ib : kTsneMaxSplit;
    int want = switch_value("TSNE_SPLIT");
    if (want < 1) want = kTsneTargetGroups / p.ib;
    if (want > most) want = most;
    if (want < 1) want = 1;
    p.tiles_per = (p.ib + want - 1) / want;
    p.S = (p.ib + p.tiles_per - 1) / p.tiles_per;
    const int64_t groups = (n + kTsneRowsPer - 1) / kTsneRowsPer;
    p.ab = (int)(groups < kTsneAttractMax ? groups : kTsneAttractMax);
    p.part_bytes = align256((size_t)p.S * (size_t)n * sizeof(float4));
    p.zpart_bytes = align256((size_t)p.ib * p.S * sizeof(double));
    p.bytes = p.part_bytes + p.zpart_bytes + align256((size_t)kTsneAttractMax * 2 * sizeof(double)) + 256 /* Z */ + 256 /* alignment */;
    return p;
}

const char* tsne_check_n(const char* who, int64_t n) {
    static thread_local char msg[160];
    if (n < 2 || n > 0x7fffff00ll) { snprintf(msg, sizeof msg, "%s: n = %lld outside 2..2^31-257", who, (long long)n); return msg; }
    return nullptr;
}

struct TsneWs { float4* part; double* zpart; double* blockpart; double* z; };

TsneWs tsne_carve(void* workspace, const TsnePlan& p) {
    char* base = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    TsneWs w;
    w.part = (float4*)base;
    w.zpart = (double*)(base + p.part_bytes);
    w.blockpart = (double*)(base + p.part_bytes + p.zpart_bytes);
    w.z = (double*)(base + p.part_bytes + p.zpart_bytes + align256((size_t)kTsneAttractMax * 2 * sizeof(double)));
    return w;
}

const char* tsne_check_csr(const char* who, int64_t n, const float* Y, const int64_t* row_off, const int32_t* col, const float* val,
                           int64_t nnz, float exaggeration) {
    static thread_local char msg[200];
    if (const char* bad = tsne_check_n(who, n)) return bad;
    if (nnz < 0 || (double)nnz > (double)n * (double)(n - 1)) {
        snprintf(msg, sizeof msg, "%s: nnz = %lld outside 0..n (n - 1): row_off[n] of a CSR without diagonal or duplicates", who, (long long)nnz);
        return msg;
    }
    if (!Y || !row_off || (nnz > 0 && (!col || !val))) { snprintf(msg, sizeof msg, "%s: null Y / row_off / col / val", who); return msg; }
    if (!std::isfinite(exaggeration) || exaggeration <= 0.f) { snprintf(msg, sizeof msg, "%s: exaggeration = %g not a positive number", who, (double)exaggeration); return msg; }
    return nullptr;
}

// one evaluation: the sweep, then the row kernel (with the descent step when y_new is given), then the record
int tsne_eval(const TsnePlan& p, const TsneWs& w, const float* Y, int64_t n, const int64_t* row_off, const int32_t* col, const float* val,
              float exaggeration, float* grad, double* z_out, float* y_new, float* update, float* gains, float momentum,
              float learning_rate, bool record, double* kl_out, double* gnorm_out, hipStream_t s) {
    hipLaunchKernelGGL(k_tsne_repulse, dim3((unsigned)p.ib, (unsigned)p.S), dim3(kTsneBlock), 0, s, (const float2*)Y, (int)n, p.tiles_per,
                       p.ib, w.part, w.zpart);
    if (int rc = check_launch("k_tsne_repulse")) return rc;
#define KGE_TSNE_ATTRACT(UPDATE, RECORD)                                                                                              \
    hipLaunchKernelGGL((k_tsne_attract<UPDATE, RECORD>), dim3((unsigned)p.ab), dim3(kTsneBlock), 0, s, (const float2*)Y, (int)n, row_off, \
                       col, val, exaggeration, (const float4*)w.part, p.S, (const double*)w.zpart, p.ib * p.S, (float2*)grad, z_out,    \
                       (float2*)y_new, (float2*)update, (float2*)gains, momentum, learning_rate, w.blockpart)
    if (y_new) { if (record) KGE_TSNE_ATTRACT(true, true); else KGE_TSNE_ATTRACT(true, false); }
    else { if (record) KGE_TSNE_ATTRACT(false, true); else KGE_TSNE_ATTRACT(false, false); }
#undef KGE_TSNE_ATTRACT
    if (int rc = check_launch("k_tsne_attract")) return rc;
    if (record) {
        hipLaunchKernelGGL(k_tsne_record, dim3(1), dim3(kTsneBlock), 0, s, (const double*)w.blockpart, p.ab, kl_out, gnorm_out);
        if (int rc = check_launch("k_tsne_record")) return rc;
    }
    return 0;
}

}  // namespace

}  // namespace kge

using namespace kge;

extern "C" {

int kge_tsne_affinities(const float* dist, const int32_t* count, int64_t n, int32_t k, float perplexity, float* cond_p, float* beta,
                        void* stream) {
    const char* who = "kge_tsne_affinities";
    if (const char* bad = tsne_check_n(who, n)) { set_error("%s", bad); return -1; }
    if (k < 1 || k > KGE_KNN_MAX) { set_error("%s: k = %d outside 1..%d (KGE_KNN_MAX)", who, (int)k, KGE_KNN_MAX); return -1; }
    if (!(perplexity >= 1.0f) || !((double)perplexity < (double)n)) {
        set_error("%s: perplexity = %g outside [1, n = %lld)", who, (double)perplexity, (long long)n);
        return -1;
    }
    if (!dist || !count || !cond_p || !beta) { set_error("%s: null dist / count / cond_p / beta", who); return -1; }
    hipLaunchKernelGGL(k_tsne_affinities, dim3((unsigned)((n + kTsneWaves - 1) / kTsneWaves)), dim3(kTsneBlock), 0, (hipStream_t)stream, dist,
                       count, n, (int)k, std::log((double)perplexity), cond_p, beta);
    return check_launch("k_tsne_affinities");
}

size_t kge_tsne_workspace_bytes(int64_t n) {
    if (tsne_check_n("kge_tsne_workspace_bytes", n)) return 0;
    return tsne_plan(n).bytes;
}

int kge_tsne_gradient(const float* Y, int64_t n, const int64_t* row_off, const int32_t* col, const float* val, int64_t nnz,
                      float exaggeration, void* workspace, size_t workspace_bytes, float* grad, double* Z, double* KL, void* stream) {
    const char* who = "kge_tsne_gradient";
    if (const char* bad = tsne_check_csr(who, n, Y, row_off, col, val, nnz, exaggeration)) { set_error("%s", bad); return -1; }
    if (!grad || !Z) { set_error("%s: null grad / Z", who); return -1; }
    const TsnePlan p = tsne_plan(n);
    if (!workspace || workspace_bytes < p.bytes) {
        set_error("%s: workspace too small (%zu bytes, kge_tsne_workspace_bytes asks for %zu)", who, workspace ? workspace_bytes : (size_t)0, p.bytes);
        return -1;
    }
    const TsneWs w = tsne_carve(workspace, p);
    return tsne_eval(p, w, Y, n, row_off, col, val, exaggeration, grad, Z, nullptr, nullptr, nullptr, 0.f, 0.f, KL != nullptr, KL, nullptr,
                     (hipStream_t)stream);
}

int kge_tsne_run(float* Y, float* Y_tmp, float* update, float* gains, int64_t n, const int64_t* row_off, const int32_t* col,
                 const float* val, int64_t nnz, int64_t it0, int64_t it1, float exaggeration, float momentum, float learning_rate,
                 int32_t record_every, double* trace, int64_t n_records, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_tsne_run";
    if (const char* bad = tsne_check_csr(who, n, Y, row_off, col, val, nnz, exaggeration)) { set_error("%s", bad); return -1; }
    if (!Y_tmp || !update || !gains) { set_error("%s: null Y_tmp / update / gains", who); return -1; }
    if (it0 < 0 || it1 < it0) { set_error("%s: iterations [%lld, %lld) are no range", who, (long long)it0, (long long)it1); return -1; }
    if (!std::isfinite(learning_rate)) { set_error("%s: learning_rate = %g is not finite", who, (double)learning_rate); return -1; }
    if (!(momentum >= 0.f && momentum < 1.f)) { set_error("%s: momentum = %g outside [0, 1)", who, (double)momentum); return -1; }
    if (record_every < 0) { set_error("%s: record_every = %d is negative (0: no records)", who, (int)record_every); return -1; }
    if (record_every > 0 && it1 / record_every > 0 && (!trace || n_records < it1 / record_every)) {
        set_error("%s: trace holds %lld records, iteration %lld needs %lld (null trace: none)", who, trace ? (long long)n_records : 0ll,
                  (long long)it1, (long long)(it1 / record_every));
        return -1;
    }
    const TsnePlan p = tsne_plan(n);
    if (!workspace || workspace_bytes < p.bytes) {
        set_error("%s: workspace too small (%zu bytes, kge_tsne_workspace_bytes asks for %zu)", who, workspace ? workspace_bytes : (size_t)0, p.bytes);
        return -1;
    }
    const TsneWs w = tsne_carve(workspace, p);
    hipStream_t s = (hipStream_t)stream;
    float* src = Y;
    float* dst = Y_tmp;
    for (int64_t it = it0; it < it1; ++it) {
        const bool record = record_every > 0 && (it + 1) % record_every == 0;
        double* slot = record ? trace + 2 * ((it + 1) / record_every - 1) : nullptr;
        if (int rc = tsne_eval(p, w, src, n, row_off, col, val, exaggeration, nullptr, w.z, dst, update, gains, momentum, learning_rate, record,
                               slot, record ? slot + 1 : nullptr, s))
            return rc;
        float* t = src; src = dst; dst = t;
    }
    if (src != Y) {   // an odd number of iterations: the state goes back to the caller's Y
        if (hipMemcpyAsync(Y, src, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
            set_error("%s: copying the state back failed", who);
            return -2;
        }
    }
    return 0;
}

}  // extern "C"
