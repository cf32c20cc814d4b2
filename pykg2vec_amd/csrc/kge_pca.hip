// kge_pca.hip -- principal component analysis of embedding rows in float64: column means, the centred Gram matrix on the float64
// matrix cores, a cyclic Jacobi eigensolver in one workgroup, and the projection of rows on the fitted axes.  No [n, dim] centred
// copy exists, no float atomic is used; for a given split every bit repeats from run to run.  DESIGN.md section 38.
//
//   k_pca_colsum        one workgroup per chunk of 64 rows: a wave per row finds the rows with a non-finite entry (they enter nothing),
//                       then a thread per column adds the chunk's valid rows in float64 in row order -> psum[chunk][dim], pcount[chunk].
//   k_pca_mean          one workgroup: a thread per column adds the chunk sums in chunk order; mean = sum / count; count.
//   k_pca_gram          a workgroup of 4 waves owns one 64 x 64 tile (ti <= tj) of the [dim, dim] output and one slab of 32-row chunks.
//                       The rows are the K dimension of v_mfma_f64_16x16x4_f64.  A chunk is loaded as float32, centred in float64 (an
//                       invalid row, a row past n and a column past dim become 0) and laid down in LDS once as s[row][column], 80
//                       doubles apart: the lane (i = lane % 16, k = lane / 16) of an operand reads s[kk + k][c0 + i], so the 32 lanes of
//                       a half-wave touch 64 different banks.  That is X^T for the A operand and X for the B operand: both come from the
//                       same slab.  A wave holds 2 x 2 accumulators of 16 x 16 over the whole slab; the next chunk is already in
//                       registers while the matrix cores run.  The tile goes to part[slab][pair][64][64].
//   k_pca_cov           a thread per element of cov: the S partials in slab order, the divisor, the lower triangle mirrored.
//   k_pca_jacobi        one workgroup of 1024 threads.  Round-robin order: ceil(dim / 2) disjoint rotations per step, dim - 1 steps per
//                       sweep (dim for odd dim, whose padding index sits out).  A step: the angles (Rutishauser's tangent) from the
//                       current a_pp, a_qq, a_pq | barrier | A <- A P on columns | barrier | A <- P^T A and V^T <- P^T V^T on rows, a_pq
//                       and a_qp set to 0 | barrier.  A and V^T live in LDS when 16 dim^2 bytes fit beside the rotation table, else in
//                       the workspace.  Stops after a sweep without a rotation, at most kPcaMaxSweeps; then the descending order (ties
//                       by index), the clamp at 0 and the sign rule.
//   k_pca_transform     a workgroup owns 16 components, which stay in LDS as the B operand [k][16] for the whole launch; tiles of 64
//                       rows stream through (grid stride), centred in float64 as s[row][k], 34 doubles apart; a wave owns 16 rows.  The
//                       accumulator is divided by sqrt(eigenvalue) where asked and rounded to float32 once.
#include <cmath>
#include <cstdio>
#include "kge_internal.h"

namespace kge {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kPcaBlock = 256;
constexpr int kPcaSumChunk = 64;       // rows per float64 partial sum of the means
constexpr int kPcaTile = 64;           // columns per side of a Gram tile
constexpr int kPcaKR = 32;             // rows per LDS fill of the Gram sweep
constexpr int kPcaLS = kPcaTile + 16;  // doubles between the rows of the slab: 160 dwords = 32 mod 64 banks
constexpr int kPcaMaxSplit = 64;
constexpr int kPcaTargetGroups = 512;  // two workgroups on each of 256 compute units
constexpr int kPcaJacBlock = 1024;
constexpr int kPcaMaxSweeps = 60;
constexpr int kPcaLdsMost = 160 * 1024 - 1024;
constexpr int kPcaTRows = 64;          // rows per tile of the transform
constexpr int kPcaTK = 32;             // dims per LDS fill of the transform
constexpr int kPcaTS = kPcaTK + 2;     // doubles between the rows of its slab: 68 dwords, 16 rows on 16 different bank quads
constexpr int kPcaTC = 16;             // components per workgroup of the transform

__device__ __forceinline__ bool pca_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-Inf

}  // namespace

__global__ void __launch_bounds__(kPcaBlock) k_pca_colsum(const float* __restrict__ rows, int64_t n, int dim, int64_t row_stride,
                                                           uint8_t* __restrict__ valid, double* __restrict__ psum,
                                                           int32_t* __restrict__ pcount) {
    __shared__ int s_valid[kPcaSumChunk];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kPcaSumChunk;
    const int here = n - r0 < kPcaSumChunk ? (int)(n - r0) : kPcaSumChunk;
    for (int r = wave; r < here; r += kPcaBlock / 64) {
        const float* __restrict__ src = rows + (r0 + r) * row_stride;
        bool bad = false;
        for (int j = lane; j < dim; j += 64) bad |= !pca_finite(src[j]);
        const bool ok = __ballot(bad) == 0ull;
        if (lane == 0) { s_valid[r] = ok ? 1 : 0; valid[r0 + r] = ok ? 1 : 0; }
    }
    __syncthreads();
    for (int c = tid; c < dim; c += kPcaBlock) {
        double s = 0.0;
        for (int r = 0; r < here; ++r)
            if (s_valid[r]) s += (double)rows[(r0 + r) * row_stride + c];
        psum[(size_t)blockIdx.x * dim + c] = s;
    }
    if (tid == 0) {
        int cnt = 0;
        for (int r = 0; r < here; ++r) cnt += s_valid[r];
        pcount[blockIdx.x] = cnt;
    }
}

__global__ void __launch_bounds__(kPcaBlock) k_pca_mean(int64_t chunks, int dim, const double* __restrict__ psum,
                                                         const int32_t* __restrict__ pcount, double* __restrict__ mean,
                                                         int32_t* __restrict__ count) {
    int cnt = 0;
    for (int64_t b = 0; b < chunks; ++b) cnt += pcount[b];
    for (int c = threadIdx.x; c < dim; c += kPcaBlock) {
        double s = 0.0;
        for (int64_t b = 0; b < chunks; ++b) s += psum[(size_t)b * dim + c];
        mean[c] = cnt > 0 ? s / (double)cnt : 0.0;
    }
    if (threadIdx.x == 0) count[0] = cnt;
}

__global__ void __launch_bounds__(kPcaBlock) k_pca_gram(const float* __restrict__ rows, int64_t n, int dim, int64_t row_stride,
                                                         const double* __restrict__ mean, const uint8_t* __restrict__ valid, int tiles,
                                                         double* __restrict__ part) {
    __shared__ double sI[kPcaKR * kPcaLS];
    __shared__ double sJ[kPcaKR * kPcaLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lk = lane >> 4;
    const int wi = wave >> 1, wj = wave & 1;
    int ti = 0, left = (int)blockIdx.x;   // the pair of the upper triangle, row by row
    while (left >= tiles - ti) { left -= tiles - ti; ++ti; }
    const int tj = ti + left;
    const int col = tid & 63, r0 = tid >> 6;
    const int ci = ti * kPcaTile + col, cj = tj * kPcaTile + col;
    const bool in_i = ci < dim, in_j = cj < dim;
    const int cic = in_i ? ci : dim - 1, cjc = in_j ? cj : dim - 1;
    const double mi = mean[cic], mj = mean[cjc];
    const int64_t chunks = (n + kPcaKR - 1) / kPcaKR;
    const int64_t c0 = chunks * blockIdx.y / gridDim.y, c1 = chunks * (blockIdx.y + 1) / gridDim.y;

    float ri[8], rj[8];
    uint32_t ok = 0;   // bit i: row r0 + 4 i of the chunk in registers is a valid row below n
    auto load_chunk = [&](int64_t c) __attribute__((always_inline)) {
        ok = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t row = c * kPcaKR + r0 + 4 * i;
            const int64_t rc = row < n ? row : n - 1;
            ok |= (row < n && valid[rc]) ? 1u << i : 0u;
            ri[i] = rows[rc * row_stride + cic];
            rj[i] = rows[rc * row_stride + cjc];
        }
    };

    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    if (c0 < c1) load_chunk(c0);
    for (int64_t c = c0; c < c1; ++c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool live = (ok >> i) & 1u;
            sI[(r0 + 4 * i) * kPcaLS + col] = live && in_i ? (double)ri[i] - mi : 0.0;
            sJ[(r0 + 4 * i) * kPcaLS + col] = live && in_j ? (double)rj[i] - mj : 0.0;
        }
        __syncthreads();
        if (c + 1 < c1) load_chunk(c + 1);
#pragma unroll
        for (int kk = 0; kk < kPcaKR; kk += 4) {
            const double a0 = sI[(kk + lk) * kPcaLS + 32 * wi + li], a1 = sI[(kk + lk) * kPcaLS + 32 * wi + 16 + li];
            const double b0 = sJ[(kk + lk) * kPcaLS + 32 * wj + li], b1 = sJ[(kk + lk) * kPcaLS + 32 * wj + 16 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();   // the slab is consumed: the next fill may overwrite it
    }
    // register r of a lane is element (4 r + lane / 16, lane % 16) of its 16 x 16 block
    double* __restrict__ dst = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kPcaTile * kPcaTile);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(32 * wi + 16 * a + 4 * r + lk) * kPcaTile + 32 * wj + 16 * b + li] = acc[a][b][r];
}

__global__ void __launch_bounds__(kPcaBlock) k_pca_cov(int dim, int tiles, int S, const double* __restrict__ part,
                                                        const int32_t* __restrict__ count, double* __restrict__ cov) {
    const int e = blockIdx.x * kPcaBlock + threadIdx.x;
    if (e >= dim * dim) return;
    const int i = e / dim, j = e - i * dim;
    const int a = i < j ? i : j, b = i < j ? j : i;
    const int ti = a / kPcaTile, tj = b / kPcaTile;
    const int pair = ti * tiles - ti * (ti - 1) / 2 + (tj - ti), pairs = tiles * (tiles + 1) / 2;
    const size_t at = (size_t)pair * (kPcaTile * kPcaTile) + (a - ti * kPcaTile) * kPcaTile + (b - tj * kPcaTile);
    double s = 0.0;
    for (int k = 0; k < S; ++k) s += part[(size_t)k * pairs * (kPcaTile * kPcaTile) + at];
    const int cnt = count[0];
    cov[e] = cnt < 2 ? 0.0 : s / (double)(cnt - 1);
}

// The matrix and the vectors may be written by one thread and read by another after a barrier: no __restrict__ on them.
template <bool LDS>
__global__ void __launch_bounds__(kPcaJacBlock) k_pca_jacobi(const double* __restrict__ cov, int dim, double* gA, double* gV,
                                                              double* __restrict__ eigenvalue, double* __restrict__ components,
                                                              int32_t* __restrict__ out_sweeps) {
    extern __shared__ double s_pca[];
    const int tid = threadIdx.x, dd = dim * dim;
    const int even = (dim + 1) & ~1, m = even >> 1, steps = even - 1;
    double* A = LDS ? s_pca : gA;
    double* V = LDS ? s_pca + dd : gV;          // row p: the vector that belongs to a_pp
    double* s_c = LDS ? s_pca + 2 * dd : s_pca;  // [m] cosines, [m] sines; later [dim] signs
    double* s_s = s_c + m;
    int* s_p = (int*)(s_c + 2 * m);              // [m] p (-1: the pair sits out), [m] q; later [dim] ranks
    int* s_q = s_p + m;
    for (int e = tid; e < dd; e += kPcaJacBlock) {
        A[e] = cov[e];
        V[e] = e / dim == e % dim ? 1.0 : 0.0;
    }
    __syncthreads();

    int sweeps = 0;
    for (;;) {
        ++sweeps;
        int rotated = 0;
        for (int step = 0; step < steps; ++step) {
            if (tid < m) {
                // the circle method: index even - 1 stays, the others turn; pair 0 is (even - 1, step)
                const int x = tid == 0 ? even - 1 : (step + tid) % steps, y = tid == 0 ? step : (step - tid + steps) % steps;
                const int p = x < y ? x : y, q = x < y ? y : x;
                double c = 1.0, s = 0.0;
                if (q < dim) {
                    const double app = A[p * dim + p], aqq = A[q * dim + q], apq = A[p * dim + q];
                    if (fabs(apq) > 0x1p-53 * sqrt(fabs(app) * fabs(aqq))) {
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                        rotated |= s != 0.0 ? 1 : 0;
                    }
                }
                s_p[tid] = s != 0.0 ? p : -1;
                s_q[tid] = q;
                s_c[tid] = c;
                s_s[tid] = s;
            }
            __syncthreads();
            for (int e = tid; e < dim * m; e += kPcaJacBlock) {   // A <- A P: columns p and q of every row
                const int i = e / m, k = e - i * m, p = s_p[k];
                if (p < 0) continue;
                const int q = s_q[k];
                const double c = s_c[k], s = s_s[k], ap = A[i * dim + p], aq = A[i * dim + q];
                A[i * dim + p] = c * ap - s * aq;
                A[i * dim + q] = s * ap + c * aq;
            }
            __syncthreads();
            for (int e = tid; e < 2 * dim * m; e += kPcaJacBlock) {   // A <- P^T A and V <- P^T V: rows p and q
                const int j = e % dim, k = (e / dim) % m, p = s_p[k];
                if (p < 0) continue;
                const bool vec = e >= dim * m;
                double* M = vec ? V : A;
                const int q = s_q[k];
                const double c = s_c[k], s = s_s[k], mp = M[p * dim + j], mq = M[q * dim + j];
                const double np = c * mp - s * mq, nq = s * mp + c * mq;
                M[p * dim + j] = !vec && j == q ? 0.0 : np;   // the rotation annihilates a_pq and a_qp
                M[q * dim + j] = !vec && j == p ? 0.0 : nq;
            }
            __syncthreads();
        }
        if (!__syncthreads_or(rotated) || sweeps == kPcaMaxSweeps) break;
    }

    // descending order, equal values by index; the sign makes the component of largest magnitude (lowest index) positive
    if (tid < dim) {
        const double mine = A[tid * dim + tid];
        int rank = 0;
        for (int j = 0; j < dim; ++j) {
            const double other = A[j * dim + j];
            rank += (other > mine || (other == mine && j < tid)) ? 1 : 0;
        }
        double big = 0.0, at = 1.0;
        for (int j = 0; j < dim; ++j) {
            const double v = V[tid * dim + j];
            if (fabs(v) > big) { big = fabs(v); at = v; }
        }
        eigenvalue[rank] = mine > 0.0 ? mine : 0.0;
        s_p[tid] = rank;
        s_c[tid] = at < 0.0 ? -1.0 : 1.0;
    }
    __syncthreads();
    for (int e = tid; e < dd; e += kPcaJacBlock) {
        const int i = e / dim, j = e - i * dim;
        components[s_p[i] * dim + j] = s_c[i] * V[e];
    }
    if (tid == 0) out_sweeps[0] = sweeps;
}

__global__ void __launch_bounds__(kPcaBlock) k_pca_transform(const float* __restrict__ rows, int64_t n, int dim, int64_t row_stride,
                                                              const double* __restrict__ mean, const double* __restrict__ components,
                                                              const double* __restrict__ eigenvalue, int n_components, int whiten,
                                                              float* __restrict__ out) {
    extern __shared__ double s_pca[];
    const int kpad = (dim + kPcaTK - 1) / kPcaTK * kPcaTK;
    double* sW = s_pca;                        // [kpad][16]: component c0 + j at column j
    double* sX = s_pca + kpad * kPcaTC;        // [64 rows][kPcaTS]
    int* s_bad = (int*)(sX + kPcaTRows * kPcaTS);   // [64]: the row holds a non-finite entry
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lk = lane >> 4;
    const int c0 = blockIdx.y * kPcaTC;
    for (int e = tid; e < kpad * kPcaTC; e += kPcaBlock) {
        const int k = e / kPcaTC, j = e - k * kPcaTC;
        sW[e] = (k < dim && c0 + j < n_components) ? components[(size_t)(c0 + j) * dim + k] : 0.0;
    }
    const int my_c = c0 + li;
    double sd = 1.0;   // whiten: sqrt(eigenvalue), 0 for a component without variance (its output is 0)
    if (whiten && my_c < n_components) { const double ev = eigenvalue[my_c]; sd = ev > 0.0 ? sqrt(ev) : 0.0; }
    const int kx = tid & 31, rx = tid >> 5;   // the fill: dim kx of rows rx + 8 i
    const int64_t row_tiles = (n + kPcaTRows - 1) / kPcaTRows;
    for (int64_t tile = blockIdx.x; tile < row_tiles; tile += gridDim.x) {
        const int64_t q0 = tile * kPcaTRows;
        __syncthreads();   // the last tile's epilogue has read s_bad (and the first fill of sW is complete below)
        if (tid < kPcaTRows) s_bad[tid] = 0;
        __syncthreads();
        f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < kpad; k0 += kPcaTK) {
            const int k = k0 + kx;
            const bool kin = k < dim;
            const double mk = mean[kin ? k : dim - 1];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t row = q0 + rx + 8 * i;
                const float v = rows[(row < n ? row : n - 1) * row_stride + (kin ? k : dim - 1)];
                const bool fin = pca_finite(v);
                if (kin && !fin) s_bad[rx + 8 * i] = 1;
                sX[(rx + 8 * i) * kPcaTS + kx] = kin && fin && row < n ? (double)v - mk : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kPcaTK; kk += 4)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sX[(16 * wave + li) * kPcaTS + kk + lk], sW[(k0 + kk + lk) * kPcaTC + li], acc, 0, 0,
                                                           0);
            __syncthreads();
        }
        // register r of a lane is row 4 r + lane / 16 of the wave's 16, component lane % 16
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lr = 16 * wave + 4 * r + lk;
            const int64_t row = q0 + lr;
            if (row < n && my_c < n_components)
                out[(size_t)row * n_components + my_c] = s_bad[lr] ? __builtin_nanf("") : (float)(sd > 0.0 ? acc[r] / sd : 0.0);
        }
    }
}

namespace {

struct PcaPlan {
    int64_t chunks;
    int tiles, pairs, S;
    bool lds;
    size_t jac_lds, o_valid, o_psum, o_pcount, o_part, o_a, o_v, bytes;
};

// The row split is a function of n and dim: enough slabs that the tile pairs fill the device; KGE_PCA_SPLIT forces it
PcaPlan pca_plan(int64_t n, int64_t dim) {
    PcaPlan p;
    p.chunks = (n + kPcaSumChunk - 1) / kPcaSumChunk;
    p.tiles = (int)((dim + kPcaTile - 1) / kPcaTile);
    p.pairs = p.tiles * (p.tiles + 1) / 2;
    int64_t want = switch_value("PCA_SPLIT");
    if (want < 1) {
        want = kPcaTargetGroups / p.pairs;
        const int64_t fills = (n + kPcaKR - 1) / kPcaKR;
        if (want > fills) want = fills;
    }
    if (want > kPcaMaxSplit) want = kPcaMaxSplit;
    if (want < 1) want = 1;
    p.S = (int)want;
    const size_t m = (size_t)((dim + 1) / 2), table = m * (2 * sizeof(double) + 2 * sizeof(int));
    p.lds = 2 * (size_t)dim * dim * sizeof(double) + table <= (size_t)kPcaLdsMost;
    p.jac_lds = (p.lds ? 2 * (size_t)dim * dim * sizeof(double) : 0) + table;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    p.o_valid = take((size_t)n);
    p.o_psum = take((size_t)p.chunks * dim * sizeof(double));
    p.o_pcount = take((size_t)p.chunks * sizeof(int32_t));
    p.o_part = take((size_t)p.S * p.pairs * kPcaTile * kPcaTile * sizeof(double));
    p.o_a = take(p.lds ? 0 : (size_t)dim * dim * sizeof(double));
    p.o_v = take(p.lds ? 0 : (size_t)dim * dim * sizeof(double));
    p.bytes = o + 256;   // + 256: the pointer is aligned up
    return p;
}

const char* pca_check(const char* who, int64_t n, int64_t dim) {
    static thread_local char msg[200];
    if (n < 1 || n > 0x7ffe0000ll) { snprintf(msg, sizeof msg, "%s: n = %lld outside 1..2^31-2^17", who, (long long)n); return msg; }
    if (dim < 1 || dim > KGE_PCA_MAX_DIM) {
        snprintf(msg, sizeof msg, "%s: dim = %lld outside 1..KGE_PCA_MAX_DIM = %d", who, (long long)dim, KGE_PCA_MAX_DIM);
        return msg;
    }
    return nullptr;
}

size_t pca_transform_lds(int64_t dim) {
    const size_t kpad = (size_t)(dim + kPcaTK - 1) / kPcaTK * kPcaTK;
    return (kpad * kPcaTC + kPcaTRows * kPcaTS) * sizeof(double) + kPcaTRows * sizeof(int);
}

// dynamic LDS above 64 KB has to be asked for, once per kernel
bool pca_lds_attr() {
    static const bool ok = [] {
        bool good = hipFuncSetAttribute((const void*)k_pca_jacobi<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kPcaLdsMost) == hipSuccess;
        good = hipFuncSetAttribute((const void*)k_pca_transform, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)pca_transform_lds(KGE_PCA_MAX_DIM)) == hipSuccess && good;
        return good;
    }();
    return ok;
}

}  // namespace

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_pca_workspace_bytes(int64_t n, int64_t dim) {
    if (pca_check("kge_pca_workspace_bytes", n, dim)) return 0;
    return pca_plan(n, dim).bytes;
}

int kge_pca_fit(const float* rows, int64_t n, int64_t dim, int64_t row_stride, void* workspace, size_t workspace_bytes, double* out_mean,
                double* out_cov, double* out_eigenvalue, double* out_components, int32_t* out_count, int32_t* out_sweeps, void* stream) {
    const char* who = "kge_pca_fit";
    if (const char* bad = pca_check(who, n, dim)) { set_error("%s", bad); return -1; }
    if (row_stride < dim) { set_error("%s: row_stride = %lld < dim = %lld", who, (long long)row_stride, (long long)dim); return -1; }
    if (!rows || !out_mean || !out_cov || !out_eigenvalue || !out_components || !out_count || !out_sweeps) {
        set_error("%s: null rows / mean / cov / eigenvalue / components / count / sweeps", who);
        return -1;
    }
    const PcaPlan p = pca_plan(n, dim);
    if (!workspace || workspace_bytes < p.bytes) {
        set_error("%s: workspace too small (%zu bytes, kge_pca_workspace_bytes asks for %zu)", who, workspace ? workspace_bytes : (size_t)0, p.bytes);
        return -1;
    }
    if (!pca_lds_attr()) { set_error("%s: the device refused %d bytes of LDS per workgroup", who, kPcaLdsMost); return -2; }
    char* base = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    uint8_t* valid = (uint8_t*)(base + p.o_valid);
    double* psum = (double*)(base + p.o_psum);
    int32_t* pcount = (int32_t*)(base + p.o_pcount);
    double* part = (double*)(base + p.o_part);
    double* ga = (double*)(base + p.o_a);
    double* gv = (double*)(base + p.o_v);
    hipStream_t s = (hipStream_t)stream;
    const int d = (int)dim;

    hipLaunchKernelGGL(k_pca_colsum, dim3((unsigned)p.chunks), dim3(kPcaBlock), 0, s, rows, n, d, row_stride, valid, psum, pcount);
    if (int rc = check_launch("k_pca_colsum")) return rc;
    hipLaunchKernelGGL(k_pca_mean, dim3(1), dim3(kPcaBlock), 0, s, p.chunks, d, (const double*)psum, (const int32_t*)pcount, out_mean, out_count);
    if (int rc = check_launch("k_pca_mean")) return rc;
    hipLaunchKernelGGL(k_pca_gram, dim3((unsigned)p.pairs, (unsigned)p.S), dim3(kPcaBlock), 0, s, rows, n, d, row_stride,
                       (const double*)out_mean, (const uint8_t*)valid, p.tiles, part);
    if (int rc = check_launch("k_pca_gram")) return rc;
    hipLaunchKernelGGL(k_pca_cov, dim3((unsigned)((d * d + kPcaBlock - 1) / kPcaBlock)), dim3(kPcaBlock), 0, s, d, p.tiles, p.S,
                       (const double*)part, (const int32_t*)out_count, out_cov);
    if (int rc = check_launch("k_pca_cov")) return rc;
    if (p.lds)
        hipLaunchKernelGGL(k_pca_jacobi<true>, dim3(1), dim3(kPcaJacBlock), p.jac_lds, s, (const double*)out_cov, d, ga, gv, out_eigenvalue,
                           out_components, out_sweeps);
    else
        hipLaunchKernelGGL(k_pca_jacobi<false>, dim3(1), dim3(kPcaJacBlock), p.jac_lds, s, (const double*)out_cov, d, ga, gv, out_eigenvalue,
                           out_components, out_sweeps);
    return check_launch("k_pca_jacobi");
}

int kge_pca_transform(const float* rows, int64_t n, int64_t dim, int64_t row_stride, const double* mean, const double* components,
                      const double* eigenvalue, int32_t n_components, int whiten, float* out, void* stream) {
    const char* who = "kge_pca_transform";
    if (const char* bad = pca_check(who, n, dim)) { set_error("%s", bad); return -1; }
    if (row_stride < dim) { set_error("%s: row_stride = %lld < dim = %lld", who, (long long)row_stride, (long long)dim); return -1; }
    if (n_components < 1 || n_components > dim) {
        set_error("%s: n_components = %d outside 1..dim = %lld", who, (int)n_components, (long long)dim);
        return -1;
    }
    if (!rows || !mean || !components || !eigenvalue || !out) { set_error("%s: null rows / mean / components / eigenvalue / out", who); return -1; }
    if (!pca_lds_attr()) { set_error("%s: the device refused %zu bytes of LDS per workgroup", who, pca_transform_lds(KGE_PCA_MAX_DIM)); return -2; }
    const int64_t row_tiles = (n + kPcaTRows - 1) / kPcaTRows;
    const dim3 grid((unsigned)(row_tiles < 1024 ? row_tiles : 1024), (unsigned)((n_components + kPcaTC - 1) / kPcaTC));
    hipLaunchKernelGGL(k_pca_transform, grid, dim3(kPcaBlock), pca_transform_lds(dim), (hipStream_t)stream, rows, n, (int)dim, row_stride, mean,
                       components, eigenvalue, (int)n_components, whiten, out);
    return check_launch("k_pca_transform");
}

}  // extern "C"
